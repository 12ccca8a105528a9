"""Voxel-grid downsampling on the device (build-added; csrc/voxel_core.hpp,
csrc/voxel.hpp; include/mcdeskew.h ``mc_voxel_*``): the step after a global deskew, when the frames
of a drive are accumulated into one cloud and most points re-observe the same surfaces.

  voxel_downsample(batch_or_rows, voxel, origin=(0, 0, 0))  -> VoxelCloud
  VoxelCloud.n_voxels, .n_points, .batch(), .rows(), .point_counts(), .keys(), .close()
  VoxelCloud.insert(batch_or_rows)  -> int, .state()  -> VoxelSums, .merge(state)  -> int
  VoxelCloud.remove(mask)  -> int, .subtract(batch_or_rows_or_state)  -> int
  VoxelCloud.normals(radius, max_nn=30, viewpoint=None, covariance=False)  -> VoxelNormals
  VoxelCloud.keep_normals(radius=None, max_nn=30), .kept_normals()  -> VoxelNormals, .kept  -> VoxelKept, .drop_normals()
  VoxelCloud.clusters(eps, min_points=10, weighted=False)  -> VoxelClusters
  VoxelCloud.segment_plane(distance_threshold, num_iterations=1000, seed=0, refine=True, among=None)  -> VoxelPlane
  VoxelCloud.select(mask, with_pcd_len=False)  -> Batch
  VoxelCloud.nearest(src, max_distance, transform=None, frame=None)  -> VoxelNearest
  VoxelCloud.register(src, max_distance, init=None, max_iterations=30, normals_radius=None, max_nn=30,
                      tol_rotation=1e-6, tol_translation=1e-6, frame=None)  -> VoxelRegistration
  VoxelCloud.register_frames(batch, max_distance, init=None, max_iterations=30, normals_radius=None, max_nn=30,
                             tol_rotation=1e-6, tol_translation=1e-6)  -> VoxelFrameRegistrations
  VoxelCloud.rays(src, origins, guard=1, max_steps=4096, frame=None)  -> VoxelRays

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

Growing a cloud (csrc/voxel.hpp "growing a live cloud"; ``mc_voxel_insert_*``, ``mc_voxel_emit_sums``,
``mc_voxel_merge_sums``): a drive is a stream, and a map is longer than one batch.  After any sequence of ``insert`` and
``merge`` calls the cloud is bit for bit what ``voxel_downsample`` returns for the concatenation of the sources in call
order: the records are integers, so adding them is exact, and voxels are numbered by first appearance, so a voxel keeps
its id and new ones follow in the order of the call's items (the points of a source in its index order; the records of
a VoxelSums in theirs, each standing for its n points arriving together).  Every item is quantised or checked on the
cloud's own grid.  ``state()`` is the cloud's records (keys, counts, the raw sums Sx, Sy, Sz, SI) and its grid as host
arrays, to be pickled or sent between ranks; ``merge`` takes one of a grid equal bit for bit.  The cloud of an empty
source, ``voxel_downsample(np.zeros((0, 4)), h, origin)``, is the way to start a map from nothing.  The cloud holds
fewer than 2^31 points in all (``n_points``).  The cost of a call is that of its items, apart from the table's growth.
Arrays returned before a call keep their first rows' identity, not their values; the next analysis sees the grown cloud.
Refused with ValueError, the cloud left bit for bit as it was: a point the filter refuses, a record with a count below
1, a key outside [-2^20, 2^20), a coordinate sum outside 0 .. n 2^32 or an intensity sum beyond +-n 2^32 (the message
names the lowest refused item), a call that would bring the cloud to 2^31 points, a batch of another context, rows that
are not (N, >= 4), a state of another grid or with arrays of the wrong dtype or shape.

Shrinking a cloud (csrc/voxel.hpp "taking voxels and points out"; ``mc_voxel_remove``, ``mc_voxel_subtract_*``): the way
out is as exact as the way in.  ``remove(mask)`` takes whole voxels out — ``remove(plane.inliers)`` is the cloud without
its ground, ``remove(labels < 0)`` the cloud without its noise — and the survivors keep their order with ids 0 .. M' - 1:
the cloud is then bit for bit ``voxel_downsample`` of its sources without the removed voxels' points.  ``subtract(src)``
takes points out: every item is quantised or checked on the cloud's grid as an insert's, its Q, QI and n leave its voxel's
record, and a voxel whose count reaches 0 leaves as in ``remove``.  ``insert(B); subtract(B)`` and ``merge(s); subtract(s)``
are the identity in every field, whatever voxels B shares with the cloud; for ``voxel_downsample(A ++ B)``, ``subtract(A)``
leaves exactly the records of ``voxel_downsample(B)``, in the relative order they had (a one-shot build may number them
differently: a voxel's first point may have been one of A's).  A frame that was corrected leaves before its correction
enters; a sliding window forgets what it inserted first.  The cloud cannot know whether the subtracted points were ever
inserted: that is the caller's contract.  Refused with ValueError, the cloud left bit for bit as it was: what ``insert`` /
``merge`` refuse of an item, an item whose voxel the cloud does not hold (the lowest item of either kind is named), a call
that brings more points than the cloud holds, and a voxel left with a record that no set of points can sum to — a count
below 0, a count of 0 with a sum that is not 0, a count n' >= 1 with a coordinate sum outside 0 .. n' 2^32 or an intensity
sum beyond +-n' 2^32 (the lowest item of such a voxel and the voxel's key are named); a mask that is not (M,) bool.  A
``subtract`` that empties no voxel costs what its items cost; ``remove``, and a ``subtract`` that empties one, cost what
the cloud costs (one pass over the survivors' records, the key table cleared and refilled; it shrinks when the survivors
fill less than an eighth of it).  Not built: tombstones (a removal that costs what leaves, at a compare in every probe
loop), ``subtract(batch, frame=f)``.

Surface normals (csrc/normals_core.hpp, csrc/normals.hpp; ``mc_voxel_normals``): what the reference's
viewer computes with open3d on every cloud without normals (read_pointcloud.py:81-84), here from the live
build and a function of the voxel set alone.  The neighbours of voxel i are the voxels of the cells within
R = ceil(radius / h) of its cell on every axis whose centroids are within the radius (i included); above
max_nn of them, the max_nn nearest by (d2, packed key) are kept.  Their offsets u = c_j - c_i give, summed
in ascending key order, the covariance C = E[u u^T] - E[u] E[u]^T; the normal is a unit eigenvector of C
for its smallest eigenvalue, the curvature its Rayleigh quotient over the trace.  Refused with ValueError:
a radius that is not finite and > 0 or exceeds 4 h, max_nn not 0 and not in 3..64, a viewpoint that is not
three finite numbers.

Kept normals (csrc/normals_core.hpp "kept normals", csrc/normals.hpp ``k_nrm_mark``; ``mc_voxel_keep_normals``): a map
changes by a frame at a time, and its normals need not be computed again as a whole for every registration.  A voxel's
row is a function of the occupied cells in the (2R + 1)^3 cell window of its cell and of their centroids, so after
``keep_normals(radius, max_nn)`` every ``insert``, ``merge``, ``subtract`` and ``remove`` computes again exactly the dirty
set D — the voxels present afterwards whose cell is within R cells, on every axis, of a touched cell: one that received
or lost an item, or was removed — and carries every other row over, on a removal to the voxel's new id.
``kept_normals()`` is then bit for bit ``normals(radius, max_nn)`` of the edited cloud, and ``kept.refreshed_last`` is
|D|.  A refused edit leaves the kept rows as they were and refreshes none.  ``register`` and ``register_frames`` read the
kept rows, and run no normals kernel, when their ``normals_radius`` (None: 2 h) and ``max_nn`` are the kept ones; with
other parameters they run as on a cloud that keeps none, and the kept rows stay.  ``normals()`` is always the full, fresh
computation.  48 bytes of device memory per voxel; ``drop_normals()`` gives them back, and a new ``voxel_downsample`` on
the context ends them.  Not built: a kept covariance or viewpoint, kept clusters.

Density clustering (csrc/cluster_core.hpp, csrc/cluster.hpp; ``mc_voxel_clusters``): DBSCAN over the live
build, the noise filtering and outlier removal of the reference's processing list (docs/Comprehensive
Guide.md:488-491) and the segmentation behind the object files its viewer opens (read_pointcloud.py:233-257).
The neighbours of a voxel are the normals' set without a cap at radius = eps; a voxel is core when it has
min_points of them (weighted: when their source points add up to min_points); a cluster is a connected
component of core voxels; a voxel that is not core joins the cluster of its core neighbour of smallest
(d2, packed key), or is noise (label -1).  Clusters are numbered 0 .. K - 1 by their lowest core voxel id, so the
partition is a function of the voxel set and the numbering of the cloud's order: the same bits on every run.
min_points = 1 is Euclidean cluster extraction (connected components).  Refused with ValueError: an eps that
is not finite and > 0 or exceeds 4 h, min_points not an integer >= 1, weighted not a bool.

Plane segmentation (csrc/plane_core.hpp, csrc/plane.hpp; ``mc_voxel_plane``): the ground filter of the reference's
processing chain (read_pointcloud.py:244-257), RANSAC as open3d's segment_plane, here defined op for op and integer
where it can be, so a VoxelPlane is the same bits on every run and equal to the NumPy restatement of
tests/planes.py.  c_v: the live build's centroids by voxel id; t the threshold; K = num_iterations; ids the
candidate voxel ids ascending (``among``: the voxels of a mask; None: all), n their number (n < 3: ValueError).
Every float64 line is one IEEE operation:

  sampler     GOLDEN = 0x9E3779B97F4A7C15;  mix(z): z = (z ^ z>>30) * 0xBF58476D1CE4E5B9;
              z = (z ^ z>>27) * 0x94D049BB133111EB; return z ^ z>>31   (uint64, wrapping)
              hypothesis k, draw j in {0, 1, 2}: r_j = mix(seed + GOLDEN * (3k + j + 1))
              a = mulhi64(r0, n);  b = mulhi64(r1, n-1), b++ if b >= a;
              c = mulhi64(r2, n-2), c++ if c >= min(a, b), then c++ if c >= max(a, b)
              p0, p1, p2 = the centroids of ids[a], ids[b], ids[c]: distinct by construction, no state
  hypothesis  e1 = p1 - p0;  e2 = p2 - p0;  n = e1 x e2, each component (u*v) - (w*x)
              l2 = (nx*nx + ny*ny) + nz*nz;  d = -((nx*p0x + ny*p0y) + nz*p0z);  tau = (t*t) * l2
              valid iff l2 > 0 and l2, d, tau are finite; an invalid hypothesis scores 0
  score       a candidate is an inlier iff s*s <= tau, s = ((nx*cx + ny*cy) + nz*cz) + d; the score is their number
  winner      the highest score of at least 3, ties to the lowest k; none: iteration -1, an all-False mask, a zero model
  refine=False  l = sqrt(l2);  n^ = n / l;  d^ = -((n^x*p0x + n^y*p0y) + n^z*p0z); the hypothesis's own inliers
  refine=True   over the voxel ids 0 .. M-1: u = c_v - p0 and ux*ux, ux*uy, ux*uz, uy*uy, uy*uz, uz*uz for an inlier,
              +0.0 otherwise; each of the nine sums is the balanced adjacent-pair tree over the leaves padded with
              +0.0 to the power of two >= max(M, 256) (``while len(a) > 1: a = a[0::2] + a[1::2]``); m = s / n_in,
              E = P / n_in, C = E - m m^T and its eigenvector as the normals compute them; q = p0 + m;
              d^ = -((n^x*qx + n^y*qy) + n^z*qz); inliers: fabs(((n^x*cx + n^y*cy) + n^z*cz) + d^) <= t; the score stays
  sign        the model is negated when the component of n^ of largest magnitude is negative (lowest axis on a tie)

The sampler draws voxel ids, so the result is a function of the cloud in its order and the seed.  Refused with
ValueError: a threshold that is not finite and > 0, num_iterations not an integer in 1..2^20, a seed not an integer
in 0..2^64-1, refine not a bool, a mask that is not (M,) bool, fewer than three candidates.

Selection (``mc_voxel_emit_selected``): ``select(mask)`` is the stable compaction of the cloud by a (M,) bool mask
into a one-frame Batch on the device, every value bit-equal to ``batch()``'s for that voxel: ``select(~plane.inliers)``
is the non-ground cloud, ``select(labels == k)`` a segment, ``select(labels >= 0)`` the outlier filter.

Registration (csrc/register_core.hpp, csrc/register.hpp; ``mc_voxel_nearest_*``, ``mc_voxel_register_*``): how well a
scan sits on the map and the small pose correction that makes it sit better, the step after motion compensation when
the IMU and GPS poses are noisy.  ``nearest`` is the nearest centroid of the live build for points that are not its
voxels; ``register`` is point-to-plane ICP on it, a VoxelRegistration equal bit for bit to the NumPy restatement of
tests/registration.py and the same on every run, the whole iteration history included.  The source is a device Batch
(its float32 x, y, z read as float64; ``frame=f``: that frame alone; None: all frames as one rigid body) or host
float64 rows (N, >= 3).  (R, t): the pose, source to cloud.  Every float64 line is one IEEE operation:

  move      q = R p + t, each component ((R0*x + R1*y) + R2*z) + t
  cell      the filter's k of q with the build's h and origin; a q that is not finite, or outside the key range, has
            no nearest voxel (id -1, dist2 inf): not an error
  nearest   W = ceil(max_distance / h); the occupied cells within W of q's cell on every axis in ascending key order;
            u = c_j - q, d2 = (ux*ux + uy*uy) + uz*uz; inside when d2 <= max_distance^2; the smallest d2 wins, ties to
            the lower cell key (cells whose box is farther than the smallest d2 known are left out: no output changes)
  pair      the winner v when ``normals(normals_radius, max_nn).counts[v] >= 3``, else none (no second choice)
  leaves    d = q - c_v;  r = (nx*dx + ny*dy) + nz*dz;  a = q x n;  J = (a, n); the upper triangle of J J^T row-major
            (21), J r (6), r r (1); +0.0 without a pair
  sums      each of the 28 by the refit's balanced adjacent-pair tree over the source point index
  step      fewer than 6 pairs: "too_few_pairs".  A x = -b by Cholesky, rows in order, inner sums ascending; a pivot
            that is not finite or not > 0: "singular".  x = (w, v).  Both return the pose before the failed step
  update    dR = the rotation of the unit quaternion (1, w/2) / |(1, w/2)| (one sqrt);  R <- dR R;  t <- dR t + v
  stop      "converged" when w.w <= tol_rotation^2 and v.v <= tol_translation^2 after the update, else
            "max_iterations" after the last one

Refused with ValueError: max_distance not finite and > 0 or beyond 4 h, a pose that is not a 4 x 4 of finite entries
with last row (0, 0, 0, 1) and |R^T R - I| <= 1e-6 in every entry, an empty source, a batch of another context, a
frame outside the batch, max_iterations not an integer in 1..2^16, a tolerance that is not finite and >= 0, and what
``normals`` refuses of normals_radius (None: 2 h) and max_nn.

Every frame of a batch (csrc/register.hpp ``k_rg_frames_*``; ``mc_voxel_register_frames``): ``register_frames`` is one
correction per frame in one call.  For every non-empty frame f, every field of result f is bit for bit what
``register(batch, max_distance, frame=f, init=init_f, ...)`` returns: a point's index is its place within its frame, so
each frame has its own tree, pair count, Cholesky step and stop, and nothing couples the frames but the cloud and its
normals, computed once per call.  All frames advance together, one launch sequence and one synchronisation per
iteration; a frame that has ended keeps the pose, history, pairs and iterations of its last evaluated iteration while
the others go on.  An empty frame is not an error: status "empty", its init as transformation, zeros elsewhere.
``ctx.transform_affine(batch, mats=r.transformations)`` is the corrected batch.  Refused with ValueError: what
``register`` refuses, a source that is not a Batch of this context, an init that is not None, one 4 x 4 or (F, 4, 4)
(the message names the frame), and F x max_iterations above 2^22 history rows.

Seeing through the cloud (csrc/rays_core.hpp, csrc/rays.hpp; ``mc_voxel_rays_*``): which voxels of the map a new scan
contradicts.  ``rays`` walks the ray of every source point, from the sensor position to the point, through the cloud's
grid and counts per voxel the rays that passed through it and the rays that ended in it; the cloud is read and never
changed.  A parked wagon that has left, a person who walked through, a ghost from a bad pose: voxels that later beams
pass and none ends in, and ``cloud.remove((r.passed >= k) & (r.ended == 0))`` carves them out.  ``through`` tells which
new points lie behind surfaces the map believes in.  The counts are integer atomic adds, the same bits on every run,
and equal to the restatement of tests/rays.py.  With h and o the cloud's; every float64 line is one IEEE operation:

  grid     per axis a, for the origin s and the endpoint e, the filter's own lines:
             as = s - o;  gs = as / h;  ks = floor(gs)        ae = e - o;  ge = ae / h;  ke = floor(ge)
           so ke is exactly the cell insert would put the point in
  skipped  a ray whose origin or endpoint the filter refuses (intensity taken as 0.0: not finite, or a key outside
           [-2^20, 2^20)), or whose walk has more than max_steps steps.  It counts nowhere, its ``through`` is -1, and it
           is counted in n_skipped: not an error, as ``nearest`` treats a point without a cell
  walk     d_a = ge_a - gs_a;  dir_a = +1 if ke_a > ks_a, -1 if ke_a < ks_a, 0 if equal;  n_a = |ke_a - ks_a|;
           steps = n_x + n_y + n_z: the walk has exactly that many transitions and always ends in ke.  The j-th crossing
           on axis a (j = 0 .. n_a - 1) has
             b = double(ks_a + j * dir_a + (dir_a > 0 ? 1 : 0));  u = b - gs_a;  t_a(j) = u / d_a
           computed afresh from j, never accumulated; an axis with all its n_a crossings done has t_a = +inf.  Each
           transition takes the axis with the smallest current t_a, ties to the lowest axis, and moves one cell along
           it.  A comparison involving a NaN cannot occur: n_a > 0 implies d_a != 0
  cells    position 0 is the origin's cell ks, position ``steps`` is ke
           ended: the voxel of ke, if the cloud holds one, gets +1
           passed: the voxels of positions 0 .. steps - 1 - guard, where the cloud holds them, get +1 each; a guard
           larger than the walk leaves none.  The cells of one walk are distinct: a ray adds at most 1 to any voxel

``guard`` is a number of cells, integer and exact: it keeps a beam that grazes the surface it ends on from carving that
surface.  Refused with ValueError: a batch of another context, rows that are not (N, >= 3), an empty source, 2^31 points
or more, a frame outside the batch or given with rows, origins that are not finite float64 of shape (3,) or (F, 3) for
a Batch, (3,) or (N, 3) for rows (the message names the shape), guard not an integer in 0..255, max_steps not an
integer in 1..2^22.  Not built: a per-point origin inside a frame of a Batch, beam divergence, occupancy probabilities.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
from ctypes import c_double, c_int32, c_int64
from typing import NamedTuple

import numpy as np

from ._lib import MC_ERR_STATE, RegisterParams, check, load, ptr
from .runtime import Batch, Context, default_context

MAX_POINTS = 2 ** 31 - 1


MAX_RADIUS_VOXELS = 4      # the neighbour search is a window of (2 ceil(radius / h) + 1)^3 <= 9^3 table probes
MAX_NN = 64


# ---- one checker per kind of argument: every method's checks come before its first touch of a device ----------------
def _number(value, name, positive=True):
    """``value`` as a finite float > 0 (``positive=False``: >= 0)."""
    bound = "> 0" if positive else ">= 0"
    try:
        x = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number {bound}, got {value!r}") from None
    if not (math.isfinite(x) and (x > 0.0 if positive else x >= 0.0)):
        raise ValueError(f"{name} must be finite and {bound}, got {value!r}")
    return x


def _window(x, name, h):
    """``x``, a search radius of a cloud of voxel size ``h`` (None: not known here, the library checks)."""
    if h is not None and x / h > MAX_RADIUS_VOXELS:
        raise ValueError(f"{name} {x!r} is {x / h:.3g} voxels of {h!r} and the search window takes at most "
                         f"{MAX_RADIUS_VOXELS}: voxelise coarser or shrink the radius")
    return x


def _integer(value, name, lo, hi, wording, also=()):
    """``value`` as an int: an integer, not a bool, in lo..hi or one of ``also``; ``wording`` says so to the caller."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not (value in also or lo <= value <= hi):
        raise ValueError(f"{name} must be {wording}, got {value!r}")
    return int(value)


def _flag(value, name):
    """A bool as 0 / 1."""
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False, got {value!r}")
    return int(bool(value))


class _Buffers(contextlib.ExitStack):
    """The device buffers of one call: each is closed on every way out of the ``with``."""

    def __init__(self, ctx):
        super().__init__()
        self._ctx = ctx

    def take(self, nbytes):
        buf = self._ctx.device_buffer(nbytes)
        self.callback(buf.close)
        return buf


def _grid(voxel, origin):
    """(h, origin as 3 float64), checked before a device is touched."""
    h = _number(voxel, "voxel")
    o = np.ascontiguousarray(origin, dtype=np.float64)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError(f"origin must be three finite numbers, got {origin!r}")
    return h, o


class VoxelNormals(NamedTuple):
    """What :meth:`VoxelCloud.normals` returns, rows in the cloud's order."""
    normals: np.ndarray             # (M, 3) float64 unit normals
    curvature: np.ndarray           # (M,) float64 surface variation l0 / (l0 + l1 + l2)
    counts: np.ndarray              # (M,) int32 neighbours used, the voxel itself included
    covariance: np.ndarray | None   # (M, 6) float64 xx, xy, xz, yy, yz, zz, when asked for


class VoxelKept(NamedTuple):
    """What :attr:`VoxelCloud.kept` returns: the parameters of the kept normals and, since the build, the work done."""
    radius: float
    max_nn: int
    full_passes: int        # the times every row was computed (keep_normals)
    refreshed_last: int     # the rows the last edit computed again: its dirty set
    refreshed_total: int    # the rows all edits computed again


def _normals_args(radius, max_nn, viewpoint, h):
    """(radius, max_nn, viewpoint as 3 float64 or None), checked before a device is touched."""
    r = _window(_number(radius, "radius"), "radius", h)
    nn = _integer(max_nn, "max_nn", 3, MAX_NN, f"0 (no cap) or an integer in 3..{MAX_NN}", also=(0,))
    vp = None
    if viewpoint is not None:
        try:
            vp = np.ascontiguousarray(viewpoint, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"viewpoint must be three finite numbers, got {viewpoint!r}") from None
        if vp.shape != (3,) or not np.isfinite(vp).all():
            raise ValueError(f"viewpoint must be three finite numbers, got {viewpoint!r}")
    return r, nn, vp


class VoxelClusters(NamedTuple):
    """What :meth:`VoxelCloud.clusters` returns: per voxel in the cloud's order, then per cluster."""
    labels: np.ndarray      # (M,) int32 the voxel's cluster 0 .. K - 1, -1 for noise
    density: np.ndarray     # (M,) int32 neighbours within eps, the voxel included (weighted: their source points)
    n_clusters: int         # K
    voxels: np.ndarray      # (K,) int32 voxels of each cluster
    points: np.ndarray      # (K,) int64 source points of each cluster
    cell_min: np.ndarray    # (K, 3) int32 the lowest kx, ky, kz of each cluster
    cell_max: np.ndarray    # (K, 3) int32 the highest


def _clusters_args(eps, min_points, weighted, h):
    """(eps, min_points, weighted as 0 / 1), checked before a device is touched."""
    e = _window(_number(eps, "eps"), "eps", h)
    return e, _integer(min_points, "min_points", 1, MAX_POINTS, "an integer >= 1"), _flag(weighted, "weighted")


MAX_ITERATIONS = 2 ** 20


class VoxelPlane(NamedTuple):
    """What :meth:`VoxelCloud.segment_plane` returns."""
    model: np.ndarray               # (4,) float64 n^x, n^y, n^z, d^: n^ . c + d^ = 0
    inliers: np.ndarray             # (M,) bool in the cloud's order
    n_inliers: int
    score: int                      # the winning hypothesis's RANSAC score, also after a refit
    iteration: int                  # the winning hypothesis k; -1: no valid hypothesis
    samples: np.ndarray             # (3,) int32 voxel ids of the winner's samples (-1 without a winner)
    covariance: np.ndarray | None   # (6,) float64 xx, xy, xz, yy, yz, zz of the refit; None when not refined
    refined: bool


def _mask_arg(mask, M, name):
    """A (M,) bool mask as contiguous bytes, checked before a device is touched."""
    if not isinstance(mask, np.ndarray) or mask.dtype != np.bool_ or mask.shape != (M,):
        raise ValueError(f"{name} must be a bool array of shape ({M},), got "
                         f"{getattr(mask, 'dtype', type(mask).__name__)} {getattr(mask, 'shape', '')}")
    return np.ascontiguousarray(mask).view(np.uint8)


def _plane_args(distance_threshold, num_iterations, seed, refine, among, M):
    """(t, K, seed, refine as 0 / 1, among as bytes or None), checked before a device is touched."""
    t = _number(distance_threshold, "distance_threshold")
    K = _integer(num_iterations, "num_iterations", 1, MAX_ITERATIONS, f"an integer in 1..{MAX_ITERATIONS}")
    sd = _integer(seed, "seed", 0, 2 ** 64 - 1, "an integer in 0..2^64-1")
    return t, K, sd, _flag(refine, "refine"), None if among is None else _mask_arg(among, M, "among")


class VoxelNearest(NamedTuple):
    """What :meth:`VoxelCloud.nearest` returns, rows in the source's point order."""
    ids: np.ndarray                 # (N,) int32 the voxel id of the nearest centroid, -1: none within max_distance
    dist2: np.ndarray               # (N,) float64 the squared distance, inf where ids is -1


class VoxelRegistration(NamedTuple):
    """What :meth:`VoxelCloud.register` returns."""
    transformation: np.ndarray      # (4, 4) float64, source to cloud
    fitness: float                  # pairs / N of the last evaluated iteration
    inlier_rmse: float              # sqrt(sum r^2 / pairs), the point-to-plane residual, of the same iteration
    pairs: int
    iterations: int                 # iterations evaluated = rows of history
    status: str                     # "converged", "max_iterations", "too_few_pairs" or "singular"
    history: np.ndarray             # (iterations, 8) float64: pairs, sum r^2, w (3), v (3); a failed step: zeros


REGISTER_STATUS = ("converged", "max_iterations", "too_few_pairs", "singular")
MAX_REGISTER_ITERATIONS = 2 ** 16
FRAME_REGISTER_STATUS = REGISTER_STATUS + ("empty",)
MAX_FRAME_HISTORY_ROWS = 2 ** 22      # F x max_iterations: 256 MB of history


class VoxelFrameRegistrations(NamedTuple):
    """What :meth:`VoxelCloud.register_frames` returns, rows in frame order; row f is ``register(..., frame=f)``."""
    transformations: np.ndarray     # (F, 4, 4) float64, source to cloud; an empty frame: its init
    fitness: np.ndarray             # (F,) float64 pairs / N_f of the frame's last evaluated iteration; empty: 0
    inlier_rmse: np.ndarray         # (F,) float64 sqrt(sum r^2 / pairs) of the same iteration; no pairs: 0
    pairs: np.ndarray               # (F,) int64
    iterations: np.ndarray          # (F,) int32 iterations evaluated
    status: np.ndarray              # (F,) int8 indices into FRAME_REGISTER_STATUS
    history: np.ndarray             # (F, max(iterations), 8) float64; rows past a frame's iterations are +0.0

    @property
    def status_names(self) -> tuple:
        return tuple(FRAME_REGISTER_STATUS[int(k)] for k in self.status)


def _distance_arg(max_distance, h):
    return _window(_number(max_distance, "max_distance"), "max_distance", h)


def _pose_arg(pose, name):
    """A 4 x 4 pose as contiguous float64 (None: the identity), checked before a device is touched."""
    if pose is None:
        return np.eye(4)
    try:
        T = np.ascontiguousarray(pose, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a 4 x 4 matrix, got {pose!r}") from None
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError(f"{name} must be a 4 x 4 matrix of finite entries, got shape {T.shape}")
    if T[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
        raise ValueError(f"{name}: the last row must be (0, 0, 0, 1), got {T[3].tolist()}")
    R = T[:3, :3]
    if not (np.abs(R.T @ R - np.eye(3)) <= 1e-6).all():
        raise ValueError(f"{name}: the rotation must be orthonormal (|R^T R - I| <= 1e-6 in every entry)")
    return T


def _source_arg(ctx, src, frame):
    """(batch, frame or -1, None) or (None, -1, rows (N, >= 3) float64), checked before a device is touched."""
    if isinstance(src, Batch):
        if src.ctx is not ctx:
            raise ValueError("the batch belongs to another context")
        f = -1
        if frame is not None:
            f = _integer(frame, "frame", 0, src.n_frames - 1, f"an integer in 0..{src.n_frames - 1}")
        n = src.n_points if f < 0 else int(src.counts[f])
        if n == 0:
            raise ValueError("the source is empty")
        if n > MAX_POINTS:
            raise ValueError(f"{n} points: a source takes fewer than 2^31")
        return src, f, None, n
    if frame is not None:
        raise ValueError("frame names a frame of a Batch; the source is rows")
    a = np.asarray(src)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError(f"rows must be (N, >= 3) = x, y, z; got shape {a.shape}")
    if a.shape[0] == 0:
        raise ValueError("the source is empty")
    if a.shape[0] > MAX_POINTS:
        raise ValueError(f"{a.shape[0]} points: a source takes fewer than 2^31")
    return None, -1, np.ascontiguousarray(a, dtype=np.float64), a.shape[0]


MAX_RAY_GUARD = 255
MAX_RAY_STEPS = 2 ** 22


class VoxelRays(NamedTuple):
    """What :meth:`VoxelCloud.rays` returns: per voxel in the cloud's order, then per ray in the source's point order."""
    passed: np.ndarray      # (M,) int32 the rays that crossed the voxel before their end (the guard cells left out)
    ended: np.ndarray       # (M,) int32 the rays whose endpoint lies in the voxel
    through: np.ndarray     # (N,) int32 the occupied voxels the ray was counted as passing; -1: the ray was skipped
    n_rays: int             # N
    n_skipped: int          # rays with an end the filter refuses, or a walk of more than max_steps steps
    steps: int              # the cell transitions of every walked ray together


def _origins_arg(origins, per, kind):
    """The sensor positions as contiguous float64 (1, 3) or (per, 3), from (3,) or (per, 3) — ``kind`` names what ``per``
    counts: the frames of a Batch or the rows — checked before a device is touched."""
    allowed = f"(3,) or ({per}, 3), one per {kind}"
    try:
        o = np.asarray(origins)
        if o.dtype.kind not in "fiu":
            raise TypeError
        o = np.ascontiguousarray(o, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"origins must be finite float64 of shape {allowed}; got {origins!r}") from None
    if o.shape != (3,) and o.shape != (per, 3):
        raise ValueError(f"origins must be finite float64 of shape {allowed}; got shape {o.shape}")
    if not np.isfinite(o).all():
        raise ValueError(f"origins must be finite float64 of shape {allowed}; got a value that is not finite")
    return o.reshape(-1, 3)


def _frame_poses_arg(init, F):
    """(F, 4, 4) float64 from None, one 4 x 4 for all frames or one per frame, each held to _pose_arg's rules."""
    if init is None:
        return np.tile(np.eye(4), (F, 1, 1))
    if isinstance(init, np.ndarray):
        per_frame = init.ndim == 3
    else:               # a sequence of matrices, which may be ragged: never made into one array
        per_frame = isinstance(init, (list, tuple)) and len(init) > 0 and np.ndim(init[0]) == 2
    if per_frame:
        if len(init) != F:
            raise ValueError(f"init must be None, one 4 x 4 matrix or one per frame ({F}, 4, 4); got {len(init)} matrices")
        out = np.empty((F, 4, 4))
        for f in range(F):
            out[f] = _pose_arg(init[f], f"init of frame {f}")
        return out
    return np.tile(_pose_arg(init, "init"), (F, 1, 1))


def _register_args(max_iterations, tol_rotation, tol_translation):
    iters = _integer(max_iterations, "max_iterations", 1, MAX_REGISTER_ITERATIONS, f"an integer in 1..{MAX_REGISTER_ITERATIONS}")
    return iters, _number(tol_rotation, "tol_rotation", positive=False), _number(tol_translation, "tol_translation", positive=False)


def plane_score_chunk() -> int:
    """The hypotheses one launch of the score phase takes (``mc_voxel_plane_chunk``); needs no device."""
    return int(load().mc_voxel_plane_chunk())


class VoxelSums(NamedTuple):
    """What :meth:`VoxelCloud.state` returns and :meth:`VoxelCloud.merge` takes: the cloud's exact records as host
    arrays in the cloud's order, and its grid.  Plain data: it pickles, and travels between ranks as it is."""
    keys: np.ndarray        # (M, 3) int32 kx, ky, kz
    counts: np.ndarray      # (M,) int32 the points of each voxel
    sums: np.ndarray        # (M, 4) int64 Sx, Sy, Sz (2^-32 voxel units inside the voxel), SI (2^-16)
    voxel: float            # the grid: records merge only into a cloud whose voxel and origin have these bits
    origin: np.ndarray      # (3,) float64


def _insert_arg(ctx, src, room):
    """(batch, None, n) or (None, rows (N, >= 4) float64, N) for a cloud with room for ``room`` more points,
    checked before a device is touched."""
    if isinstance(src, Batch):
        if src.ctx is not ctx:
            raise ValueError("the batch belongs to another context")
        batch, rows, n = src, None, src.n_points
    else:
        a = np.asarray(src)
        if a.ndim != 2 or a.shape[1] < 4:
            raise ValueError(f"rows must be (N, >= 4) = x, y, z, intensity; got shape {a.shape}")
        try:
            batch, rows, n = None, np.ascontiguousarray(a, dtype=np.float64), a.shape[0]
        except (TypeError, ValueError):
            raise ValueError(f"rows must be numbers, got dtype {a.dtype}") from None
    if n > room:
        raise ValueError(f"the cloud holds {MAX_POINTS - room} points and the call brings {n}: a cloud takes fewer than "
                         f"2^31 in all")
    return batch, rows, n


def _same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def _sums_arg(state, h, origin):
    """(keys, counts, sums) of a VoxelSums of this very grid, contiguous, checked before a device is touched."""
    try:
        keys, counts, sums, voxel, o = state.keys, state.counts, state.sums, state.voxel, state.origin
    except AttributeError:
        raise ValueError(f"merge takes a VoxelSums (keys, counts, sums, voxel, origin), got {type(state).__name__}") from None
    if h is None or origin is None:
        raise ValueError("this cloud does not know its grid: merge needs a cloud made by voxel_downsample")
    if not isinstance(voxel, (float, np.floating)) or not _same_bits(voxel, h):
        raise ValueError(f"the state's voxel {voxel!r} is not the cloud's {h!r} bit for bit: a different grid")
    if not isinstance(o, np.ndarray) or o.dtype != np.float64 or o.shape != (3,) or not _same_bits(o, origin):
        raise ValueError(f"the state's origin {o!r} is not the cloud's {origin!r} bit for bit: a different grid")
    for a, name, dtype, tail in ((keys, "keys", np.int32, (3,)), (counts, "counts", np.int32, ()), (sums, "sums", np.int64, (4,))):
        if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape[1:] != tail or a.ndim != 1 + len(tail):
            raise ValueError(f"state.{name} must be a {np.dtype(dtype).name} array of shape (M{''.join(f', {t}' for t in tail)}), "
                             f"got {getattr(a, 'dtype', type(a).__name__)} {getattr(a, 'shape', '')}")
    if not len(keys) == len(counts) == len(sums):
        raise ValueError(f"state.keys, .counts and .sums must hold the same M records, got {len(keys)}, {len(counts)}, {len(sums)}")
    if len(keys) > MAX_POINTS:
        raise ValueError(f"{len(keys)} records: a merge takes fewer than 2^31")
    return np.ascontiguousarray(keys), np.ascontiguousarray(counts), np.ascontiguousarray(sums)


class VoxelCloud:
    """What the last :func:`voxel_downsample` of a context left on the device.  The outputs are produced
    on demand from the per-voxel sums, any number of times; :meth:`insert` and :meth:`merge` grow it in place;
    the next ``voxel_downsample`` on the same context (or :meth:`close`) ends this object's validity."""

    def __init__(self, ctx: Context, n_voxels: int, generation: int, voxel: float | None = None, origin=None,
                 n_points: int | None = None):
        self.ctx, self.n_voxels, self._gen, self._h = ctx, int(n_voxels), generation, voxel
        self._origin = None if origin is None else np.array(origin, np.float64)
        self.n_points = n_points        # N: the points the cloud holds (None: made by hand, the library knows)

    def _live(self):
        if self.ctx._voxel_gen != self._gen:
            raise ValueError("this VoxelCloud is closed or was replaced by a later voxel_downsample on its context")

    def _room(self):
        return MAX_POINTS - (self.n_points or 0)

    def _grown(self, n_new):
        """After an insert or a merge: M and N from the call and the library."""
        self.n_voxels += int(n_new)
        n = c_int64(0)
        check(self.ctx.lib.mc_voxel_points(self.ctx.handle, ctypes.byref(n)), "voxel points")
        self.n_points = n.value
        return int(n_new)

    def insert(self, src) -> int:
        """The points of ``src`` — a device Batch of the cloud's context, or host float64 rows (N, >= 4) — into the
        cloud, on its own grid: afterwards the cloud is bit for bit ``voxel_downsample`` of everything it was given,
        in call order (module docstring; include/mcdeskew.h ``mc_voxel_insert_*``).  Voxels keep their ids; new ones
        follow.  -> the number of new voxels.  A refused point raises ValueError naming it and changes nothing."""
        batch, rows, n = _insert_arg(self.ctx, src, self._room())
        self._live()
        if n == 0:
            return 0
        ctx = self.ctx
        m = c_int64(0)
        if batch is not None:
            bf, bi = c_int32(-1), c_int64(-1)
            check(ctx.lib.mc_voxel_insert_batch(ctx.handle, batch.handle, ctypes.byref(m), ctypes.byref(bf), ctypes.byref(bi)),
                  "insert")
        else:
            with _Buffers(ctx) as bufs:
                d_rows = bufs.take(rows.nbytes)
                d_rows.from_host(rows)
                bad = c_int64(-1)
                check(ctx.lib.mc_voxel_insert_f64(ctx.handle, d_rows.ptr, rows.shape[1], n, ctypes.byref(m), ctypes.byref(bad)),
                      "insert")
        return self._grown(m.value)

    def state(self) -> "VoxelSums":
        """The cloud's exact records and its grid as host arrays (``mc_voxel_emit_sums``): merging them into a cloud
        of the same grid equals inserting the points they stand for."""
        self._live()
        M = self.n_voxels
        sums = np.zeros((0, 4), np.int64)
        if M:
            with _Buffers(self.ctx) as bufs:
                buf = bufs.take(32 * M)
                check(self.ctx.lib.mc_voxel_emit_sums(self.ctx.handle, buf.ptr), "state")
                sums = buf.to_host(np.int64, count=4 * M).reshape(M, 4)
        return VoxelSums(self.keys(), self.point_counts(), sums, float(self._h), np.array(self._origin, np.float64))

    def merge(self, state) -> int:
        """The records of ``state`` (a :class:`VoxelSums` of this very grid, voxel and origin equal bit for bit) into
        the cloud, each as the points it stands for arriving together (module docstring; ``mc_voxel_merge_sums``):
        afterwards the cloud is ``voxel_downsample`` of this cloud's points followed by the state's.  -> the number of
        new voxels.  A refused record raises ValueError naming it and changes nothing."""
        keys, counts, sums = _sums_arg(state, self._h, self._origin)
        self._live()
        m = len(keys)
        if m == 0:
            return 0
        ctx = self.ctx
        with _Buffers(ctx) as bufs:
            d = [bufs.take(a.nbytes) for a in (keys, counts, sums)]
            for buf, a in zip(d, (keys, counts, sums)):
                buf.from_host(a)
            new, bad = c_int64(0), c_int64(-1)
            check(ctx.lib.mc_voxel_merge_sums(ctx.handle, d[0].ptr, d[1].ptr, d[2].ptr, m, ctypes.byref(new), ctypes.byref(bad)),
                  "merge")
        return self._grown(new.value)

    def _shrunk(self, n_gone):
        """After a remove or a subtract: M and N from the call and the library."""
        self.n_voxels -= int(n_gone)
        n = c_int64(0)
        check(self.ctx.lib.mc_voxel_points(self.ctx.handle, ctypes.byref(n)), "voxel points")
        self.n_points = n.value
        return int(n_gone)

    def remove(self, mask) -> int:
        """The voxels whose ``mask`` entry is True — a (M,) bool in the cloud's order, as ``segment_plane(...).inliers``
        or ``clusters(...).labels < 0`` — out of the cloud (module docstring; include/mcdeskew.h ``mc_voxel_remove``).
        The survivors keep their order and get ids 0 .. M' - 1: afterwards the cloud is bit for bit
        ``voxel_downsample`` of its sources without the removed voxels' points.  -> the number of voxels removed.
        An all-False mask touches nothing.  The cost is that of the cloud, not of what leaves."""
        m = _mask_arg(mask, self.n_voxels, "mask")
        self._live()
        if len(m) == 0:
            return 0
        ctx = self.ctx
        with _Buffers(ctx) as bufs:
            buf = bufs.take(len(m))
            buf.from_host(m)
            gone = c_int64(0)
            check(ctx.lib.mc_voxel_remove(ctx.handle, buf.ptr, ctypes.byref(gone)), "remove")
        return self._shrunk(gone.value)

    def subtract(self, src) -> int:
        """The points of ``src`` — a device Batch of the cloud's context, host float64 rows (N, >= 4), or a
        :class:`VoxelSums` of this very grid, each record standing for its n points — out of the cloud, on its own
        grid (module docstring; include/mcdeskew.h ``mc_voxel_subtract_*``).  ``insert(src)`` then ``subtract(src)``
        is the identity, bit for bit; a voxel whose count reaches 0 leaves as in :meth:`remove`.  -> the number of
        voxels that became empty and left.  The cloud cannot know whether the points were ever inserted: that they
        were is the caller's contract, and only what cannot be true is refused — a point the filter refuses, a voxel
        the cloud does not hold, more points than the cloud or a voxel holds, a sum no remaining points can have —
        with ValueError naming the lowest such item, the cloud left bit for bit as it was."""
        why = c_int32(0)
        ctx = self.ctx
        gone = c_int64(0)
        if hasattr(src, "sums") and hasattr(src, "voxel"):
            keys, counts, sums = _sums_arg(src, self._h, self._origin)
            self._live()
            if len(keys) == 0:
                return 0
            with _Buffers(ctx) as bufs:
                d = [bufs.take(a.nbytes) for a in (keys, counts, sums)]
                for buf, a in zip(d, (keys, counts, sums)):
                    buf.from_host(a)
                bad = c_int64(-1)
                check(ctx.lib.mc_voxel_subtract_sums(ctx.handle, d[0].ptr, d[1].ptr, d[2].ptr, len(keys), ctypes.byref(gone),
                                                     ctypes.byref(bad), ctypes.byref(why)), "subtract")
            return self._shrunk(gone.value)
        batch, rows, n = _insert_arg(ctx, src, MAX_POINTS)
        self._live()
        if n == 0:
            return 0
        if batch is not None:
            bf, bi = c_int32(-1), c_int64(-1)
            check(ctx.lib.mc_voxel_subtract_batch(ctx.handle, batch.handle, ctypes.byref(gone), ctypes.byref(bf), ctypes.byref(bi),
                                                  ctypes.byref(why)), "subtract")
        else:
            with _Buffers(ctx) as bufs:
                d_rows = bufs.take(rows.nbytes)
                d_rows.from_host(rows)
                bad = c_int64(-1)
                check(ctx.lib.mc_voxel_subtract_f64(ctx.handle, d_rows.ptr, rows.shape[1], n, ctypes.byref(gone), ctypes.byref(bad),
                                                    ctypes.byref(why)), "subtract")
        return self._shrunk(gone.value)

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
        with _Buffers(self.ctx) as bufs:
            buf = bufs.take(n * np.dtype(dtype).itemsize)
            args = [None, None, None]
            args[which] = buf.ptr
            check(self.ctx.lib.mc_voxel_emit_f64(self.ctx.handle, *args), "voxel_downsample")
            a = buf.to_host(dtype, count=n)
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

    def normals(self, radius, max_nn: int = 30, viewpoint=None, covariance: bool = False) -> "VoxelNormals":
        """Surface normals of the voxel points, the reference viewer's
        ``estimate_normals(KDTreeSearchParamHybrid(radius=0.1, max_nn=30))`` (read_pointcloud.py:81-84) as a
        function of the voxel set alone (module docstring; include/mcdeskew.h ``mc_voxel_normals``).  Rows in
        the cloud's order, as :meth:`rows` / :meth:`keys`; any number of calls, with any radii, on one live
        cloud.  ``max_nn`` 0: no cap.  ``viewpoint``: normals face it; None: the component of largest
        magnitude is positive.  A voxel with fewer than three neighbours (itself included) gets (0, 0, 1) and
        curvature 0, and its count says so."""
        r, nn, vp = _normals_args(radius, max_nn, viewpoint, self._h)
        self._live()
        M = self.n_voxels
        if M == 0:
            return VoxelNormals(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.int32), np.zeros((0, 6)) if covariance else None)
        ctx = self.ctx
        with _Buffers(ctx) as bufs:
            d_out, d_counts, d_cov = bufs.take(M * 32), bufs.take(M * 4), bufs.take(M * 48) if covariance else None
            check(ctx.lib.mc_voxel_normals(ctx.handle, r, nn, ptr(vp, c_double), d_out.ptr, d_counts.ptr,
                                           d_cov.ptr if covariance else None), "normals")
            out = d_out.to_host(np.float64, count=4 * M).reshape(M, 4)
            counts = d_counts.to_host(np.int32, count=M)
            cov = d_cov.to_host(np.float64, count=6 * M).reshape(M, 6) if covariance else None
        return VoxelNormals(np.ascontiguousarray(out[:, :3]), np.ascontiguousarray(out[:, 3]), counts, cov)

    def keep_normals(self, radius=None, max_nn: int = 30) -> None:
        """Compute ``normals(radius, max_nn)`` now, once, and keep the rows on the device across every later
        :meth:`insert`, :meth:`merge`, :meth:`subtract` and :meth:`remove` (module docstring "Kept normals";
        include/mcdeskew.h ``mc_voxel_keep_normals``): an edit computes again only the rows it can change, and
        :meth:`kept_normals` stays bit for bit a fresh :meth:`normals`.  ``radius`` None: 2 h, the default of
        :meth:`register`, which reads the kept rows when its ``normals_radius`` and ``max_nn`` are these.  Called
        again, it replaces what was kept."""
        if radius is None:
            if self._h is None:
                raise ValueError("radius=None means twice the voxel size, which this cloud does not know")
            radius = 2 * self._h
        r, nn, _ = _normals_args(radius, max_nn, None, self._h)
        self._live()
        check(self.ctx.lib.mc_voxel_keep_normals(self.ctx.handle, r, nn), "keep_normals")

    def kept_normals(self) -> "VoxelNormals":
        """The kept rows as :meth:`normals` returns them (covariance None): no normals kernel runs.  ValueError when the
        cloud keeps none."""
        self._live()
        if self.kept is None:
            raise ValueError("this cloud keeps no normals: call keep_normals first")
        M = self.n_voxels
        if M == 0:
            return VoxelNormals(np.zeros((0, 3)), np.zeros(0), np.zeros(0, np.int32), None)
        ctx = self.ctx
        with _Buffers(ctx) as bufs:
            d_out, d_counts = bufs.take(M * 32), bufs.take(M * 4)
            check(ctx.lib.mc_voxel_kept_normals(ctx.handle, d_out.ptr, d_counts.ptr), "kept_normals")
            out = d_out.to_host(np.float64, count=4 * M).reshape(M, 4)
            counts = d_counts.to_host(np.int32, count=M)
        return VoxelNormals(np.ascontiguousarray(out[:, :3]), np.ascontiguousarray(out[:, 3]), counts, None)

    @property
    def kept(self) -> "VoxelKept | None":
        """What the cloud keeps (``mc_voxel_kept_info``): the parameters and the counters, or None when it keeps no
        normals.  A cloud that an edit left without a live build (a failure that was no refusal) keeps none either and
        reads as None here; its next use raises."""
        self._live()
        radius, nn, counters = c_double(0.0), c_int32(0), (c_int64 * 3)()
        rc = self.ctx.lib.mc_voxel_kept_info(self.ctx.handle, ctypes.byref(radius), ctypes.byref(nn), counters)
        if rc == MC_ERR_STATE:
            return None
        check(rc, "kept")
        return VoxelKept(radius.value, nn.value, int(counters[0]), int(counters[1]), int(counters[2]))

    def drop_normals(self) -> None:
        """Keep no normals any more and give their device memory back (``mc_voxel_drop_normals``); the edits and
        :meth:`register` then behave as on a cloud that never kept any."""
        self._live()
        check(self.ctx.lib.mc_voxel_drop_normals(self.ctx.handle), "drop_normals")

    def clusters(self, eps, min_points: int = 10, weighted: bool = False) -> "VoxelClusters":
        """DBSCAN over the voxel points (module docstring; include/mcdeskew.h ``mc_voxel_clusters``): labels
        and densities in the cloud's order, as :meth:`rows` / :meth:`keys`, and per cluster its voxels, source
        points and cell bounding box.  Noise is label -1: ``labels >= 0`` is the radius-outlier filter, and
        ``cloud.rows()[labels == k]`` is segment k.  ``weighted``: the density of a voxel is the number of
        source points of its neighbours, not the number of neighbours.  Any number of calls, with any
        parameters, on one live cloud."""
        e, mp, w = _clusters_args(eps, min_points, weighted, self._h)
        self._live()
        M = self.n_voxels
        if M == 0:
            return VoxelClusters(np.zeros(0, np.int32), np.zeros(0, np.int32), 0, np.zeros(0, np.int32), np.zeros(0, np.int64),
                                 np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32))
        ctx = self.ctx
        with _Buffers(ctx) as bufs:
            d_labels, d_density = bufs.take(M * 4), bufs.take(M * 4)
            k = c_int64(0)
            check(ctx.lib.mc_voxel_clusters(ctx.handle, e, mp, w, d_labels.ptr, d_density.ptr, ctypes.byref(k)), "clusters")
            K = k.value
            labels = d_labels.to_host(np.int32, count=M)
            density = d_density.to_host(np.int32, count=M)
            if K == 0:
                return VoxelClusters(labels, density, 0, np.zeros(0, np.int32), np.zeros(0, np.int64),
                                     np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32))
            # one buffer, the int64 array first: voxels (K,), points (K,), cell_min (K, 3), cell_max (K, 3)
            d_stats = bufs.take(K * 36)
            base = d_stats.ptr.value
            check(ctx.lib.mc_voxel_cluster_stats(ctx.handle, base + 8 * K, base, base + 12 * K, base + 24 * K), "clusters")
            raw = d_stats.to_host(np.int32, count=9 * K)
        return VoxelClusters(labels, density, K, np.ascontiguousarray(raw[2 * K:3 * K]),
                             np.ascontiguousarray(raw[:2 * K]).view(np.int64), np.ascontiguousarray(raw[3 * K:6 * K]).reshape(K, 3),
                             np.ascontiguousarray(raw[6 * K:]).reshape(K, 3))

    def segment_plane(self, distance_threshold, num_iterations: int = 1000, seed: int = 0, refine: bool = True,
                      among=None) -> "VoxelPlane":
        """RANSAC plane segmentation of the voxel points, open3d's ``segment_plane(distance_threshold, 3,
        num_iterations)`` as a function of the cloud in its order and the seed (module docstring; include/mcdeskew.h
        ``mc_voxel_plane``).  ``refine``: the model is refitted on the winner's inliers and the inliers are taken
        again.  ``among``: a (M,) bool mask of the candidates — ``among=~ground.inliers`` finds the next plane.  Any
        number of calls on one live cloud."""
        M = self.n_voxels
        t, K, sd, rf, cand = _plane_args(distance_threshold, num_iterations, seed, refine, among, M)
        self._live()
        if (M if cand is None else int(np.count_nonzero(cand))) < 3:
            raise ValueError("a plane needs three candidate voxels")
        ctx = self.ctx
        with _Buffers(ctx) as bufs:
            d_inliers, d_among = bufs.take(M), bufs.take(M) if cand is not None else None
            if cand is not None:
                d_among.from_host(cand)
            model, cov = np.zeros(4), np.zeros(6)
            samples, stats = np.zeros(3, np.int32), np.zeros(4, np.int64)
            check(ctx.lib.mc_voxel_plane(ctx.handle, t, K, sd, rf, d_among.ptr if cand is not None else None, d_inliers.ptr,
                                         ptr(model, c_double), ptr(cov, c_double), ptr(samples, c_int32), ptr(stats, c_int64)),
                  "segment_plane")
            inliers = d_inliers.to_host(np.uint8, count=M).view(np.bool_)
        refined = bool(stats[3])
        return VoxelPlane(model, inliers, int(stats[2]), int(stats[1]), int(stats[0]), samples, cov if refined else None, refined)

    def select(self, mask, with_pcd_len: bool = False) -> Batch:
        """The voxel points whose ``mask`` entry is True, in the cloud's order, as a one-frame float32 Batch like
        :meth:`batch`'s (every value bit-equal to it), compacted on the device (``mc_voxel_emit_selected``)."""
        m = _mask_arg(mask, self.n_voxels, "mask")
        self._live()
        ctx = self.ctx
        out = Batch(ctx, [int(np.count_nonzero(m))], with_pcd_len=with_pcd_len)
        with _Buffers(ctx) as bufs:
            buf = bufs.take(max(len(m), 1))
            if len(m):
                buf.from_host(m)
            check(ctx.lib.mc_voxel_emit_selected(ctx.handle, buf.ptr, out.handle), "select")
        return out

    def nearest(self, src, max_distance, transform=None, frame=None) -> "VoxelNearest":
        """The nearest centroid of the cloud to every point of ``src`` moved by ``transform`` (4 x 4, source to
        cloud; None: the identity), within ``max_distance`` <= 4 h (module docstring; include/mcdeskew.h
        ``mc_voxel_nearest_*``).  ``src``: a device Batch (``frame=f``: that frame alone) or host float64 rows
        (N, >= 3).  Rows in the source's point order; the cloud is not changed."""
        d = _distance_arg(max_distance, self._h)
        T = _pose_arg(transform, "transform")
        batch, f, rows, n = _source_arg(self.ctx, src, frame)
        self._live()
        ctx = self.ctx
        with _Buffers(ctx) as bufs:
            d_ids, d_dist2 = bufs.take(4 * n), bufs.take(8 * n)
            if batch is not None:
                rc = ctx.lib.mc_voxel_nearest_batch(ctx.handle, batch.handle, f, d, ptr(T, c_double), d_ids.ptr, d_dist2.ptr)
            else:
                d_rows = bufs.take(rows.nbytes)
                d_rows.from_host(rows)
                rc = ctx.lib.mc_voxel_nearest_f64(ctx.handle, d_rows.ptr, rows.shape[1], n, d, ptr(T, c_double), d_ids.ptr,
                                                  d_dist2.ptr)
            check(rc, "nearest")
            return VoxelNearest(d_ids.to_host(np.int32, count=n), d_dist2.to_host(np.float64, count=n))

    def register(self, src, max_distance, init=None, max_iterations: int = 30, normals_radius=None, max_nn: int = 30,
                 tol_rotation: float = 1e-6, tol_translation: float = 1e-6, frame=None) -> "VoxelRegistration":
        """Point-to-plane ICP of ``src`` against the cloud from the pose ``init`` (4 x 4, source to cloud; None: the
        identity): per iteration the nearest centroid within ``max_distance`` <= 4 h of every moved point, the
        cloud's normals (``normals(normals_radius, max_nn)``, computed once per call on the device;
        ``normals_radius`` None: 2 h), the 6 x 6 normal equations summed by a tree over the point index, and a
        Cholesky step (module docstring; include/mcdeskew.h ``mc_voxel_register_*``).  A Batch moves as one rigid
        body (``frame=f``: that frame alone).  The cloud is not changed; any number of calls on one live cloud."""
        d = _distance_arg(max_distance, self._h)
        T = _pose_arg(init, "init")
        iters, tol_r, tol_t = _register_args(max_iterations, tol_rotation, tol_translation)
        if normals_radius is None:
            if self._h is None:
                raise ValueError("normals_radius=None means twice the voxel size, which this cloud does not know")
            normals_radius = 2 * self._h
        radius, nn, _ = _normals_args(normals_radius, max_nn, None, self._h)
        batch, f, rows, n = _source_arg(self.ctx, src, frame)
        self._live()
        ctx = self.ctx
        par = RegisterParams(d, radius, tol_r, tol_t, (c_double * 16)(*T.reshape(-1).tolist()), nn, iters)
        out, history, stats = np.zeros((4, 4)), np.zeros((iters, 8)), np.zeros(4, np.int64)
        tail = (ctypes.byref(par), ptr(out, c_double), ptr(history, c_double), ptr(stats, c_int64))
        with _Buffers(ctx) as bufs:
            if batch is not None:
                rc = ctx.lib.mc_voxel_register_batch(ctx.handle, batch.handle, f, *tail)
            else:
                d_rows = bufs.take(rows.nbytes)
                d_rows.from_host(rows)
                rc = ctx.lib.mc_voxel_register_f64(ctx.handle, d_rows.ptr, rows.shape[1], n, *tail)
            check(rc, "register")
        pairs, done = int(stats[0]), int(stats[1])
        history = np.ascontiguousarray(history[:done])
        rmse = math.sqrt(float(history[-1, 1]) / pairs) if pairs else 0.0
        return VoxelRegistration(out, pairs / n, rmse, pairs, done, REGISTER_STATUS[int(stats[2])], history)

    def register_frames(self, batch, max_distance, init=None, max_iterations: int = 30, normals_radius=None, max_nn: int = 30,
                        tol_rotation: float = 1e-6, tol_translation: float = 1e-6) -> "VoxelFrameRegistrations":
        """:meth:`register` of every frame of ``batch`` on its own, in one call: row f of the result is bit for bit
        ``register(batch, max_distance, frame=f, init=init_f, ...)`` (module docstring; include/mcdeskew.h
        ``mc_voxel_register_frames``).  ``init``: None, one 4 x 4 for all frames, or (F, 4, 4).  The normals are
        computed once; the frames advance together, and one that has ended is left as it ended.  An empty frame
        gets the status "empty".  ``ctx.transform_affine(batch, mats=result.transformations)`` applies the result."""
        d = _distance_arg(max_distance, self._h)
        if not isinstance(batch, Batch):
            raise ValueError("register_frames takes a Batch: one registration per frame (rows have no frames)")
        if batch.ctx is not self.ctx:
            raise ValueError("the batch belongs to another context")
        F = batch.n_frames
        T = _frame_poses_arg(init, F)
        iters, tol_r, tol_t = _register_args(max_iterations, tol_rotation, tol_translation)
        if F * iters > MAX_FRAME_HISTORY_ROWS:
            raise ValueError(f"{F} frames x max_iterations {iters} is more than 2^22 history rows (256 MB): lower max_iterations")
        if normals_radius is None:
            if self._h is None:
                raise ValueError("normals_radius=None means twice the voxel size, which this cloud does not know")
            normals_radius = 2 * self._h
        radius, nn, _ = _normals_args(normals_radius, max_nn, None, self._h)
        counts = np.asarray(batch.counts, np.int64).reshape(-1)
        if len(counts) and int(counts.max()) > MAX_POINTS:
            raise ValueError(f"{int(counts.max())} points in a frame: a source takes fewer than 2^31")
        self._live()
        ctx = self.ctx
        par = RegisterParams(d, radius, tol_r, tol_t, (c_double * 16)(*np.eye(4).reshape(-1).tolist()), nn, iters)
        out, history, stats = np.zeros((F, 4, 4)), np.zeros((F, iters, 8)), np.zeros((F, 4), np.int64)
        check(ctx.lib.mc_voxel_register_frames(ctx.handle, batch.handle, ctypes.byref(par), ptr(T, c_double), ptr(out, c_double),
                                               ptr(history, c_double), ptr(stats, c_int64)), "register_frames")
        pairs, done = stats[:, 0].copy(), stats[:, 1].astype(np.int32)
        last = history[np.arange(F), np.maximum(done - 1, 0), 1]
        # per frame what register computes: pairs / N_f and math.sqrt(sum r^2 / pairs), both on Python floats
        fitness = np.array([int(p) / int(n) if n else 0.0 for p, n in zip(pairs, counts)], np.float64)
        rmse = np.array([math.sqrt(float(s) / int(p)) if p else 0.0 for s, p in zip(last, pairs)], np.float64)
        history = np.ascontiguousarray(history[:, :int(done.max()) if F else 0])
        return VoxelFrameRegistrations(out, fitness, rmse, pairs, done, stats[:, 2].astype(np.int8), history)

    def rays(self, src, origins, guard: int = 1, max_steps: int = 4096, frame=None) -> "VoxelRays":
        """The ray of every point of ``src``, from its sensor position to the point, walked through the cloud's grid:
        per voxel the rays that passed through it and the rays that ended in it, per ray the occupied voxels it passed
        (module docstring "Seeing through the cloud"; include/mcdeskew.h ``mc_voxel_rays_*``).  ``src``: a device Batch
        (``frame=f``: that frame alone) or host float64 rows (N, >= 3).  ``origins``: the sensor positions, already in
        the cloud's frame: (3,) for all, or (F, 3), one per frame of a Batch, or (N, 3), one per row.  ``guard``: the
        last cells before a ray's end that do not count as passed, so a beam that grazes the surface it ends on does
        not carve it.  A ray with an end outside the grid, or of more than ``max_steps`` cells, is skipped: its
        ``through`` is -1.  The intended use is ``cloud.remove((r.passed >= k) & (r.ended == 0))``: the voxels that k
        beams saw through and none stopped in.  The cloud is not changed; any number of calls on one live cloud."""
        batch, f, rows, n = _source_arg(self.ctx, src, frame)
        o = _origins_arg(origins, batch.n_frames, "frame") if batch is not None else _origins_arg(origins, n, "row")
        g = _integer(guard, "guard", 0, MAX_RAY_GUARD, f"an integer in 0..{MAX_RAY_GUARD}")
        ms = _integer(max_steps, "max_steps", 1, MAX_RAY_STEPS, f"an integer in 1..{MAX_RAY_STEPS}")
        self._live()
        ctx, M = self.ctx, self.n_voxels
        stats = np.zeros(4, np.int64)
        with _Buffers(ctx) as bufs:
            d_passed, d_ended, d_through = bufs.take(4 * max(M, 1)), bufs.take(4 * max(M, 1)), bufs.take(4 * n)
            tail = (g, ms, d_passed.ptr, d_ended.ptr, d_through.ptr, ptr(stats, c_int64))
            if batch is not None:
                rc = ctx.lib.mc_voxel_rays_batch(ctx.handle, batch.handle, f, ptr(o, c_double), len(o), *tail)
            else:
                d_rows, d_origins = bufs.take(rows.nbytes), bufs.take(o.nbytes)
                d_rows.from_host(rows)
                d_origins.from_host(o)
                rc = ctx.lib.mc_voxel_rays_f64(ctx.handle, d_rows.ptr, rows.shape[1], n, d_origins.ptr, len(o), *tail)
            check(rc, "rays")
            empty = np.zeros(0, np.int32)
            return VoxelRays(d_passed.to_host(np.int32, count=M) if M else empty,
                             d_ended.to_host(np.int32, count=M) if M else empty.copy(),
                             d_through.to_host(np.int32, count=n), int(stats[0]), int(stats[1]), int(stats[2]))

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
        with _Buffers(ctx) as bufs:
            d_rows = bufs.take(max(a.nbytes, 8))
            if a.size:
                d_rows.from_host(a)
            bad = c_int64(-1)
            check(ctx.lib.mc_voxel_build_f64(ctx.handle, d_rows.ptr, a.shape[1], a.shape[0], h, ptr(o, c_double),
                                             ctypes.byref(m), ctypes.byref(bad)), "voxel_downsample")
    ctx._voxel_serial += 1
    ctx._voxel_gen = ctx._voxel_serial
    return VoxelCloud(ctx, m.value, ctx._voxel_gen, h, o, src.n_points if isinstance(src, Batch) else a.shape[0])
