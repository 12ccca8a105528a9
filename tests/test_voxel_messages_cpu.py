"""Every ValueError of voxel.py that needs no device, held to its whole text: one refused call or more per ``raise``,
through ``VoxelCloud(_NoDevice(), 10, 7, 0.05)`` and ``voxel_downsample``, each compared with ``==``.  The strings were
recorded from the module as it stood before its argument checks were folded into shared helpers, so a helper that
rewords a message, drops the ``!r`` of the offending value or chains the conversion error fails here.

A source Batch is stood in for by an object of the class that never ran its constructor (the checks read its
context, frame sizes and point count only), and 2^31 rows by a broadcast view of one row, so the size limits are
reachable too.  Not reachable without a device, and so not in the table: ``DeviceBuffer.from_host``'s "array larger
than the device buffer" and the ValueError ``check`` makes of a return code of the library (runtime.py and _lib.py,
not voxel.py); in voxel.py itself every ``raise`` has a row."""
import numpy as np
import pytest

from conftest import pkg


class _NoDevice:
    """Stands where a Context would: any use of the library fails the test."""
    _voxel_gen = 7

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name}) before the arguments were checked")


CTX = _NoDevice()
ROWS = np.zeros((5, 3))
ROWS4 = np.zeros((5, 4))
HUGE3 = np.broadcast_to(np.zeros((1, 3)), (2 ** 31, 3))
HUGE4 = np.broadcast_to(np.zeros((1, 4)), (2 ** 31, 4))
BAD_LAST = np.eye(4)
BAD_LAST[3, 0] = 0.5
SKEW = np.eye(4)
SKEW[0, 1] = 2e-6
NOT_FINITE = np.eye(4)
NOT_FINITE[0, 3] = np.nan
TWO = np.zeros(10, np.bool_)
TWO[[2, 5]] = True


def _batch(m, ctx, counts, n_points=None):
    b = object.__new__(m.Batch)
    b.ctx, b.counts, b.n_frames = ctx, np.asarray(counts, np.int64), len(counts)
    b.n_points = int(sum(counts)) if n_points is None else n_points
    return b


def _cloud(m):
    return m.VoxelCloud(CTX, 10, 7, 0.05)


# (what is refused, the call given the package, the whole message)
TABLE = [
    # ---- voxel_downsample -------------------------------------------------------------------------------------------
    ("voxel not a number", lambda m: m.voxel_downsample(ROWS4, "x"), "voxel must be a number > 0, got 'x'"),
    ("voxel None", lambda m: m.voxel_downsample(ROWS4, None), "voxel must be a number > 0, got None"),
    ("voxel zero", lambda m: m.voxel_downsample(ROWS4, 0), "voxel must be finite and > 0, got 0"),
    ("voxel nan", lambda m: m.voxel_downsample(ROWS4, float("nan")), "voxel must be finite and > 0, got nan"),
    ("origin short", lambda m: m.voxel_downsample(ROWS4, 0.1, origin=(0, 0)), "origin must be three finite numbers, got (0, 0)"),
    ("origin inf", lambda m: m.voxel_downsample(ROWS4, 0.1, origin=[0.0, float("inf"), 0.0]),
     "origin must be three finite numbers, got [0.0, inf, 0.0]"),
    ("build: batch of another context", lambda m: m.voxel_downsample(_batch(m, CTX, [3]), 0.1, context=_NoDevice()),
     "the batch belongs to another context"),
    ("build: batch of 2^31 points", lambda m: m.voxel_downsample(_batch(m, CTX, [3], 2 ** 31), 0.1),
     "2147483648 points: the voxel filter takes fewer than 2^31"),
    ("build: rows of three columns", lambda m: m.voxel_downsample(ROWS, 0.1),
     "rows must be (N, >= 4) = x, y, z, intensity; got shape (5, 3)"),
    ("build: rows of one axis", lambda m: m.voxel_downsample(np.zeros(5), 0.1),
     "rows must be (N, >= 4) = x, y, z, intensity; got shape (5,)"),
    ("build: 2^31 rows", lambda m: m.voxel_downsample(HUGE4, 0.1), "2147483648 points: the voxel filter takes fewer than 2^31"),
    # ---- the liveness of a cloud ------------------------------------------------------------------------------------
    ("closed cloud", lambda m: m.VoxelCloud(CTX, 10, 6, 0.05).rows(),
     "this VoxelCloud is closed or was replaced by a later voxel_downsample on its context"),
    ("closed cloud, after the checks", lambda m: m.VoxelCloud(CTX, 10, 6, 0.05).normals(0.1),
     "this VoxelCloud is closed or was replaced by a later voxel_downsample on its context"),
    # ---- normals ----------------------------------------------------------------------------------------------------
    ("radius not a number", lambda m: _cloud(m).normals("x"), "radius must be a number > 0, got 'x'"),
    ("radius None", lambda m: _cloud(m).normals(None), "radius must be a number > 0, got None"),
    ("radius negative", lambda m: _cloud(m).normals(-0.1), "radius must be finite and > 0, got -0.1"),
    ("radius inf", lambda m: _cloud(m).normals(float("inf")), "radius must be finite and > 0, got inf"),
    ("radius over the window", lambda m: _cloud(m).normals(0.3),
     "radius 0.3 is 6 voxels of 0.05 and the search window takes at most 4: voxelise coarser or shrink the radius"),
    ("radius just over the window", lambda m: _cloud(m).normals(0.2001),
     "radius 0.2001 is 4 voxels of 0.05 and the search window takes at most 4: voxelise coarser or shrink the radius"),
    ("max_nn 2", lambda m: _cloud(m).normals(0.1, max_nn=2), "max_nn must be 0 (no cap) or an integer in 3..64, got 2"),
    ("max_nn 65", lambda m: _cloud(m).normals(0.1, max_nn=65), "max_nn must be 0 (no cap) or an integer in 3..64, got 65"),
    ("max_nn a bool", lambda m: _cloud(m).normals(0.1, max_nn=True), "max_nn must be 0 (no cap) or an integer in 3..64, got True"),
    ("max_nn a float", lambda m: _cloud(m).normals(0.1, max_nn=30.0), "max_nn must be 0 (no cap) or an integer in 3..64, got 30.0"),
    ("viewpoint not numbers", lambda m: _cloud(m).normals(0.1, viewpoint="abc"), "viewpoint must be three finite numbers, got 'abc'"),
    ("viewpoint of two", lambda m: _cloud(m).normals(0.1, viewpoint=(1.0, 2.0)), "viewpoint must be three finite numbers, got (1.0, 2.0)"),
    ("viewpoint nan", lambda m: _cloud(m).normals(0.1, viewpoint=[0.0, 0.0, float("nan")]),
     "viewpoint must be three finite numbers, got [0.0, 0.0, nan]"),
    # ---- clusters ---------------------------------------------------------------------------------------------------
    ("eps not a number", lambda m: _cloud(m).clusters("x"), "eps must be a number > 0, got 'x'"),
    ("eps zero", lambda m: _cloud(m).clusters(0.0), "eps must be finite and > 0, got 0.0"),
    ("eps over the window", lambda m: _cloud(m).clusters(0.25),
     "eps 0.25 is 5 voxels of 0.05 and the search window takes at most 4: voxelise coarser or shrink the radius"),
    ("min_points zero", lambda m: _cloud(m).clusters(0.1, min_points=0), "min_points must be an integer >= 1, got 0"),
    ("min_points a bool", lambda m: _cloud(m).clusters(0.1, min_points=True), "min_points must be an integer >= 1, got True"),
    ("min_points 2^31", lambda m: _cloud(m).clusters(0.1, min_points=2 ** 31), "min_points must be an integer >= 1, got 2147483648"),
    ("weighted an int", lambda m: _cloud(m).clusters(0.1, weighted=1), "weighted must be True or False, got 1"),
    ("weighted None", lambda m: _cloud(m).clusters(0.1, weighted=None), "weighted must be True or False, got None"),
    # ---- segment_plane ----------------------------------------------------------------------------------------------
    ("threshold not a number", lambda m: _cloud(m).segment_plane([1]), "distance_threshold must be a number > 0, got [1]"),
    ("threshold zero", lambda m: _cloud(m).segment_plane(0), "distance_threshold must be finite and > 0, got 0"),
    ("num_iterations zero", lambda m: _cloud(m).segment_plane(0.1, num_iterations=0),
     "num_iterations must be an integer in 1..1048576, got 0"),
    ("num_iterations over", lambda m: _cloud(m).segment_plane(0.1, num_iterations=2 ** 20 + 1),
     "num_iterations must be an integer in 1..1048576, got 1048577"),
    ("num_iterations a bool", lambda m: _cloud(m).segment_plane(0.1, num_iterations=True),
     "num_iterations must be an integer in 1..1048576, got True"),
    ("seed negative", lambda m: _cloud(m).segment_plane(0.1, seed=-1), "seed must be an integer in 0..2^64-1, got -1"),
    ("seed 2^64", lambda m: _cloud(m).segment_plane(0.1, seed=2 ** 64), "seed must be an integer in 0..2^64-1, got 18446744073709551616"),
    ("seed a float", lambda m: _cloud(m).segment_plane(0.1, seed=1.5), "seed must be an integer in 0..2^64-1, got 1.5"),
    ("refine an int", lambda m: _cloud(m).segment_plane(0.1, refine=0), "refine must be True or False, got 0"),
    ("among of floats", lambda m: _cloud(m).segment_plane(0.1, among=np.zeros(10)),
     "among must be a bool array of shape (10,), got float64 (10,)"),
    ("among too long", lambda m: _cloud(m).segment_plane(0.1, among=np.zeros(11, np.bool_)),
     "among must be a bool array of shape (10,), got bool (11,)"),
    ("among a list", lambda m: _cloud(m).segment_plane(0.1, among=[True] * 10), "among must be a bool array of shape (10,), got list "),
    ("among of two voxels", lambda m: _cloud(m).segment_plane(0.1, among=TWO), "a plane needs three candidate voxels"),
    ("a cloud of two voxels", lambda m: m.VoxelCloud(CTX, 2, 7, 0.05).segment_plane(0.1), "a plane needs three candidate voxels"),
    # ---- select -----------------------------------------------------------------------------------------------------
    ("mask of bytes", lambda m: _cloud(m).select(np.zeros(10, np.uint8)), "mask must be a bool array of shape (10,), got uint8 (10,)"),
    ("mask of two axes", lambda m: _cloud(m).select(np.zeros((10, 1), np.bool_)),
     "mask must be a bool array of shape (10,), got bool (10, 1)"),
    # ---- nearest and register: the window, the pose, the source ----------------------------------------------------
    ("max_distance not a number", lambda m: _cloud(m).nearest(ROWS, "x"), "max_distance must be a number > 0, got 'x'"),
    ("max_distance nan", lambda m: _cloud(m).register(ROWS, float("nan")), "max_distance must be finite and > 0, got nan"),
    ("max_distance over the window", lambda m: _cloud(m).nearest(ROWS, 0.5),
     "max_distance 0.5 is 10 voxels of 0.05 and the search window takes at most 4: voxelise coarser or shrink the radius"),
    ("transform not a matrix", lambda m: _cloud(m).nearest(ROWS, 0.1, transform="x"), "transform must be a 4 x 4 matrix, got 'x'"),
    ("init 3 x 3", lambda m: _cloud(m).register(ROWS, 0.1, init=np.eye(3)), "init must be a 4 x 4 matrix of finite entries, got shape (3, 3)"),
    ("transform not finite", lambda m: _cloud(m).nearest(ROWS, 0.1, transform=NOT_FINITE),
     "transform must be a 4 x 4 matrix of finite entries, got shape (4, 4)"),
    ("transform last row", lambda m: _cloud(m).nearest(ROWS, 0.1, transform=BAD_LAST),
     "transform: the last row must be (0, 0, 0, 1), got [0.5, 0.0, 0.0, 1.0]"),
    ("init not orthonormal", lambda m: _cloud(m).register(ROWS, 0.1, init=SKEW),
     "init: the rotation must be orthonormal (|R^T R - I| <= 1e-6 in every entry)"),
    ("source batch of another context", lambda m: _cloud(m).nearest(_batch(m, _NoDevice(), [3]), 0.1),
     "the batch belongs to another context"),
    ("frame beyond the batch", lambda m: _cloud(m).nearest(_batch(m, CTX, [3, 4]), 0.1, frame=2), "frame must be an integer in 0..1, got 2"),
    ("frame a bool", lambda m: _cloud(m).register(_batch(m, CTX, [3, 4]), 0.1, frame=True), "frame must be an integer in 0..1, got True"),
    ("empty frame", lambda m: _cloud(m).nearest(_batch(m, CTX, [3, 0]), 0.1, frame=1), "the source is empty"),
    ("empty batch", lambda m: _cloud(m).register(_batch(m, CTX, [0, 0]), 0.1), "the source is empty"),
    ("source batch of 2^31 points", lambda m: _cloud(m).nearest(_batch(m, CTX, [3], 2 ** 31), 0.1),
     "2147483648 points: a source takes fewer than 2^31"),
    ("frame with rows", lambda m: _cloud(m).nearest(ROWS, 0.1, frame=0), "frame names a frame of a Batch; the source is rows"),
    ("source rows of two columns", lambda m: _cloud(m).nearest(np.zeros((5, 2)), 0.1), "rows must be (N, >= 3) = x, y, z; got shape (5, 2)"),
    ("no source rows", lambda m: _cloud(m).register(np.zeros((0, 3)), 0.1), "the source is empty"),
    ("2^31 source rows", lambda m: _cloud(m).nearest(HUGE3, 0.1), "2147483648 points: a source takes fewer than 2^31"),
    # ---- register's own ---------------------------------------------------------------------------------------------
    ("max_iterations zero", lambda m: _cloud(m).register(ROWS, 0.1, max_iterations=0), "max_iterations must be an integer in 1..65536, got 0"),
    ("max_iterations a float", lambda m: _cloud(m).register(ROWS, 0.1, max_iterations=3.0),
     "max_iterations must be an integer in 1..65536, got 3.0"),
    ("max_iterations over", lambda m: _cloud(m).register(ROWS, 0.1, max_iterations=2 ** 16 + 1),
     "max_iterations must be an integer in 1..65536, got 65537"),
    ("tol_rotation not a number", lambda m: _cloud(m).register(ROWS, 0.1, tol_rotation="x"), "tol_rotation must be a number >= 0, got 'x'"),
    ("tol_rotation negative", lambda m: _cloud(m).register(ROWS, 0.1, tol_rotation=-1e-9), "tol_rotation must be finite and >= 0, got -1e-09"),
    ("tol_translation None", lambda m: _cloud(m).register(ROWS, 0.1, tol_translation=None), "tol_translation must be a number >= 0, got None"),
    ("tol_translation inf", lambda m: _cloud(m).register(ROWS, 0.1, tol_translation=float("inf")),
     "tol_translation must be finite and >= 0, got inf"),
    ("normals_radius of a cloud without h", lambda m: m.VoxelCloud(CTX, 10, 7).register(ROWS, 0.1),
     "normals_radius=None means twice the voxel size, which this cloud does not know"),
    ("normals_radius over the window", lambda m: _cloud(m).register(ROWS, 0.1, normals_radius=0.3),
     "radius 0.3 is 6 voxels of 0.05 and the search window takes at most 4: voxelise coarser or shrink the radius"),
    ("normals_radius zero", lambda m: _cloud(m).register(ROWS, 0.1, normals_radius=0), "radius must be finite and > 0, got 0"),
    ("register max_nn", lambda m: _cloud(m).register(ROWS, 0.1, max_nn=2), "max_nn must be 0 (no cap) or an integer in 3..64, got 2"),
]


# the rows whose call fails in a conversion: the message is raised ``from None``, the conversion's own error not shown
FROM_NONE = {"voxel not a number", "voxel None", "radius not a number", "radius None", "viewpoint not numbers", "eps not a number",
             "threshold not a number", "max_distance not a number", "transform not a matrix", "tol_rotation not a number",
             "tol_translation None"}


@pytest.mark.parametrize("what,call,message", TABLE, ids=[row[0] for row in TABLE])
def test_whole_message(what, call, message):
    with pytest.raises(ValueError) as e:
        call(pkg())
    assert str(e.value) == message
    assert e.value.__cause__ is None and e.value.__suppress_context__ == (what in FROM_NONE)


def test_the_table_is_whole():
    labels = [row[0] for row in TABLE]
    assert len(set(labels)) == len(labels) >= 50 and FROM_NONE <= set(labels)
