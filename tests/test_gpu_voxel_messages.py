"""What the library says when it refuses a call of the voxel analyses after it has looked up the state: the return
code and the whole text of mc_last_error, for calls straight into the library on one built cloud of a few hundred
voxels and on a context without a build.  The expected strings are the format strings of csrc/voxel.hip written
out by hand (%g of 2.5 is "2.5"), so a helper that rewords one, or an entry point whose first failing check is
no longer the one it was, fails here."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = 0.5
WINDOW = " voxels of 0.5 and the search window takes at most 4: voxelise coarser or shrink the radius"


def refused(mc, lib, rc, code, text):
    assert rc == code and lib.mc_last_error().decode() == text, (rc, lib.mc_last_error())


def register_tail(mc, init=None, max_distance=1.0):
    """(params, then the transformation, history and stats the call writes) of a mc_voxel_register_*"""
    T = np.eye(4) if init is None else init
    par = mc._lib.RegisterParams(max_distance, 1.0, 1e-6, 1e-6, (ctypes.c_double * 16)(*T.reshape(-1).tolist()), 30, 2)
    out, history, stats = np.zeros(16), np.zeros(16), np.zeros(4, np.int64)
    p, cd = mc._lib.ptr, mc._lib.c_double
    return par, (ctypes.byref(par), p(out, cd), p(history, cd), p(stats, mc._lib.c_int64))


def test_refusals_after_the_state_lookup(mc):
    lib, p, cd = mc._lib.load(), mc._lib.ptr, mc._lib.c_double
    INVALID, STATE = mc._lib.MC_ERR_INVALID, mc._lib.MC_ERR_STATE
    ctx = mc.Context(0)
    h = ctx.handle
    rng = np.random.default_rng(21)
    rows = np.column_stack([rng.uniform(-4.0, 4.0, (400, 3)), rng.uniform(0.0, 255.0, 400)]).astype(np.float32).astype(np.float64)
    cloud = mc.voxel_downsample(rows, H, context=ctx)
    M = cloud.n_voxels
    assert 200 < M <= 400
    d_rows = ctx.device_buffer(rows.nbytes)
    d_rows.from_host(rows)
    big = ctx.device_buffer(48 * M + 16)        # any output of M voxels
    ids = ctx.device_buffer(8 * len(rows))
    src = ctx.batch([100, 0, 300])
    src.upload_aos(rows)
    model, cov, samples, stats = np.zeros(4), np.zeros(6), np.zeros(3, np.int32), np.zeros(4, np.int64)
    plane_out = (p(model, cd), p(cov, cd), p(samples, mc._lib.c_int32), p(stats, mc._lib.c_int64))
    eye = np.eye(4)

    # a window over 4 h, by each of its three names
    refused(mc, lib, lib.mc_voxel_normals(h, 2.5, 30, None, big.ptr, None, None), INVALID, "radius 2.5 is 5" + WINDOW)
    refused(mc, lib, lib.mc_voxel_clusters(h, 2.25, 3, 0, big.ptr, None, None), INVALID, "eps 2.25 is 4.5" + WINDOW)
    refused(mc, lib, lib.mc_voxel_nearest_f64(h, d_rows.ptr, 4, len(rows), 3.0, p(eye, cd), ids.ptr, big.ptr), INVALID,
            "max_distance 3 is 6" + WINDOW)
    par, tail = register_tail(mc, max_distance=2.125)
    refused(mc, lib, lib.mc_voxel_register_batch(h, src.handle, -1, *tail), INVALID, "max_distance 2.125 is 4.25" + WINDOW)
    # the normals' own arguments
    refused(mc, lib, lib.mc_voxel_normals(h, 1.0, 2, None, big.ptr, None, None), INVALID, "max_nn must be 0 (no cap) or in 3..64 (got 2)")
    refused(mc, lib, lib.mc_voxel_normals(h, 1.0, 30, None, big.ptr.value + 8, None, None), INVALID,
            "d_normals and d_cov must be 16-byte aligned")
    # the plane's
    refused(mc, lib, lib.mc_voxel_plane(h, 0.2, 0, 0, 1, None, big.ptr, *plane_out), INVALID,
            "num_iterations must be in 1..1048576 (got 0)")
    two = np.zeros(M, np.uint8)
    two[[1, M - 1]] = 1
    among = ctx.device_buffer(M)
    among.from_host(two)
    refused(mc, lib, lib.mc_voxel_plane(h, 0.2, 16, 0, 1, among.ptr, big.ptr, *plane_out), INVALID,
            "a plane needs three candidate voxels (the mask has 2)")
    # an out batch of the wrong size, for both emits
    out = ctx.batch([M + 1])
    refused(mc, lib, lib.mc_voxel_emit_batch(h, out.handle), INVALID,
            f"the out batch must be one frame of exactly {M} points (it has 1 frames, {M + 1} points)")
    refused(mc, lib, lib.mc_voxel_emit_selected(h, among.ptr, out.handle), INVALID,
            f"the out batch must be one frame of exactly 2 points (it has 1 frames, {M + 1} points)")
    refused(mc, lib, lib.mc_voxel_emit_selected(h, among.ptr, src.handle), INVALID,
            "the out batch must be one frame of exactly 2 points (it has 3 frames, 400 points)")
    # the poses
    bad_last = np.eye(4)
    bad_last[3, 0] = 0.5
    refused(mc, lib, lib.mc_voxel_nearest_f64(h, d_rows.ptr, 4, len(rows), 1.0, p(bad_last, cd), ids.ptr, big.ptr), INVALID,
            "transform: the last row must be 0, 0, 0, 1")
    scaled = np.eye(4)
    scaled[:3, :3] *= 1.001
    par, tail = register_tail(mc, init=scaled)
    refused(mc, lib, lib.mc_voxel_register_f64(h, d_rows.ptr, 4, len(rows), *tail), INVALID,
            "init: the entries must be finite and the rotation orthonormal (|R^T R - I| <= 1e-6)")
    # a frame past the batch's
    refused(mc, lib, lib.mc_voxel_nearest_batch(h, src.handle, 3, 1.0, p(eye, cd), ids.ptr, big.ptr), INVALID,
            "frame 3 of a batch of 3 frames")
    par, tail = register_tail(mc)
    refused(mc, lib, lib.mc_voxel_register_batch(h, src.handle, 3, *tail), INVALID, "frame 3 of a batch of 3 frames")
    # the build is live and no clustering of it exists
    refused(mc, lib, lib.mc_voxel_cluster_stats(h, big.ptr, None, None, None), STATE,
            "mc_voxel_cluster_stats needs a successful mc_voxel_clusters of the live build first")

    # every entry on a context without a build (every check before the lookup passes)
    cloud.close()
    needs = " needs a successful mc_voxel_build_* first"
    one = ctx.batch([2])
    calls = {
        "mc_voxel_emit_batch": lambda: lib.mc_voxel_emit_batch(h, one.handle),
        "mc_voxel_emit_f64": lambda: lib.mc_voxel_emit_f64(h, big.ptr, None, None),
        "mc_voxel_normals": lambda: lib.mc_voxel_normals(h, 1.0, 30, None, big.ptr, None, None),
        "mc_voxel_clusters": lambda: lib.mc_voxel_clusters(h, 1.0, 3, 0, big.ptr, None, None),
        "mc_voxel_plane": lambda: lib.mc_voxel_plane(h, 0.2, 16, 0, 1, None, big.ptr, *plane_out),
        "mc_voxel_emit_selected": lambda: lib.mc_voxel_emit_selected(h, among.ptr, one.handle),
        "mc_voxel_nearest_batch": lambda: lib.mc_voxel_nearest_batch(h, src.handle, 0, 1.0, p(eye, cd), ids.ptr, big.ptr),
        "mc_voxel_nearest_f64": lambda: lib.mc_voxel_nearest_f64(h, d_rows.ptr, 4, len(rows), 1.0, p(eye, cd), ids.ptr, big.ptr),
        "mc_voxel_register_batch": lambda: lib.mc_voxel_register_batch(h, src.handle, -1, *tail),
        "mc_voxel_register_f64": lambda: lib.mc_voxel_register_f64(h, d_rows.ptr, 4, len(rows), *tail),
    }
    for name, call in calls.items():
        refused(mc, lib, call(), STATE, name + needs)
    refused(mc, lib, lib.mc_voxel_cluster_stats(h, big.ptr, None, None, None), STATE,
            "mc_voxel_cluster_stats needs a successful mc_voxel_clusters of the live build first")
    # the same on a context that never had one
    bare = mc.Context(0)
    refused(mc, lib, lib.mc_voxel_normals(bare.handle, 1.0, 30, None, None, None, None), STATE, "mc_voxel_normals" + needs)
    refused(mc, lib, lib.mc_voxel_emit_f64(bare.handle, None, None, None), STATE, "mc_voxel_emit_f64" + needs)
    bare.close()
    for b in (d_rows, big, ids, among, src, out, one):
        b.close()
    gc.collect()
    ctx.close()
