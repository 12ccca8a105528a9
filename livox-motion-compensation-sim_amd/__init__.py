"""MI355X-native LiDAR motion compensation — the hot path of
manishborikar92/livox-motion-compensation-sim, rebuilt on hand-written gfx950 HIP kernels.

Import with ``importlib.import_module("livox-motion-compensation-sim_amd")`` (the directory
name carries hyphens) or via the repo-root helper ``mcamd.py``.

Drop-in surface (reference file:line in each docstring):
  LiDARMotionSimulator   lidar_motion_compensation.py:274-859 (config contract, pose tables,
                         transform_pointcloud, batched frame loop, merge)
  MotionCompensator      livox_mid70_complete_simulator.py:1426-1536 (+ driver 2086-2105)
  LiDARSimulator         livox_mid70_complete_simulator.py:990-1171 (+ driver 2028-2084): the
                         ray-march scanner that produces MotionCompensator's frames
  LiDARPoint, IMUData    livox_mid70_complete_simulator.py:97-129
  LivoxLVXWriter, codecs lidar_motion_compensation.py:24-272, 932-948 (byte-exact LVX / PCD)
  CoordinateTransformer  livox_mid70_complete_simulator.py:145-233, 2107-2180 (coords)
  csim_export            livox_mid70_complete_simulator.py:235-374, 1603-1715: its LivoxLVXWriter
                         (lvx / lvx2 / lvx3), DataExporter (PCD / XYZ / CSV) and DeviceInfo, byte-exact
                         (the top-level LivoxLVXWriter stays the LMC one)
  ingest                 the inverse of both writers: read_lvx / read_lvx_batch (LVX v1.1, CSIM lvx /
                         lvx2 / lvx3) and read_points / read_points_batch (ASCII PCD / XYZ / CSV)
                         decoded on the device into rows or a Batch
  las                    LAS 1.2 without laspy (lidar_motion_compensation.py:950-963,
                         livox_mid70_complete_simulator.py:1671-1698): encode_las / write_las from rows
                         or a Batch, read_las / read_las_batch back, records packed and unpacked on the device
  voxel                  build-added: voxel_downsample(batch or rows, voxel, origin) -> VoxelCloud, the voxel-grid
                         filter after a global deskew, with integer sums: bit-identical on every run;
                         VoxelCloud.insert(batch or rows) / .state() -> VoxelSums / .merge(state): the cloud grown in
                         place, bit for bit the one-shot cloud of the concatenated sources;
                         VoxelCloud.normals(radius, max_nn=30, viewpoint, covariance) -> VoxelNormals, the viewer's
                         estimate_normals (read_pointcloud.py:81-84) from the live build, a function of the voxel set;
                         VoxelCloud.clusters(eps, min_points=10, weighted) -> VoxelClusters, DBSCAN over the live build:
                         noise removal and segmentation (docs/Comprehensive Guide.md:488-491), the same on every run;
                         VoxelCloud.segment_plane(distance_threshold, num_iterations=1000, seed=0, refine, among)
                         -> VoxelPlane, RANSAC plane segmentation (the ground filter of read_pointcloud.py:244-257), and
                         VoxelCloud.select(mask) -> Batch, the cloud cut by a mask on the device;
                         VoxelCloud.nearest(src, max_distance, transform, frame) -> VoxelNearest and
                         VoxelCloud.register(src, max_distance, init, ...) -> VoxelRegistration, a scan registered
                         against the cloud by point-to-plane ICP, the whole iteration history the same on every run;
                         VoxelCloud.register_frames(batch, max_distance, init, ...) -> VoxelFrameRegistrations, every
                         frame of a batch registered on its own in one call, row f bit for bit register(..., frame=f);
                         VoxelCloud.keep_normals(radius=None, max_nn=30), .kept_normals() -> VoxelNormals, .kept ->
                         VoxelKept, .drop_normals(): the normals kept across insert / merge / subtract / remove, only the
                         rows an edit can change computed again, bit for bit a fresh normals(); register* read them;
                         VoxelCloud.rays(src, origins, guard=1, max_steps=4096, frame) -> VoxelRays, the rays of a scan
                         walked through the cloud: per voxel the beams that passed it and that ended in it (free-space
                         carving: remove((passed >= k) & (ended == 0))), integer counts, the same on every run
Device layer: Context, Batch (blocked-CSR float32 columns in HBM); multi-GPU: dist.
"""
from . import _lib, codecs, config, coords, csim_export, dist, ingest, las, raymarch, runtime, trajectory, voxel  # noqa: F401
from .csim_export import DataExporter, DeviceInfo  # noqa: F401
from .ingest import read_lvx, read_lvx_batch, read_points, read_points_batch  # noqa: F401
from .las import LasData, encode_las, read_las, read_las_batch, write_las  # noqa: F401
from .coords import CoordinateSystem, CoordinateTransformer, GPSData  # noqa: F401
from .codecs import LivoxLVXWriter  # noqa: F401
from ._lib import McError, McLibraryError  # noqa: F401
from .compensator import IMUData, LiDARPoint, MotionCompensator, imu_to_arrays  # noqa: F401
from .config import default_config, validate_config  # noqa: F401
from .raymarch import LiDARSimulator  # noqa: F401
from .runtime import Batch, Context, default_context  # noqa: F401
from .simulator import LiDARMotionSimulator  # noqa: F401
from .voxel import (VoxelCloud, VoxelClusters, VoxelFrameRegistrations, VoxelKept, VoxelNearest, VoxelNormals,  # noqa: F401
                    VoxelPlane, VoxelRays, VoxelRegistration, VoxelSums, voxel_downsample)  # noqa: F401

__version__ = "0.1.0"
