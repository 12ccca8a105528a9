/*
 * mcdeskew.h — C-ABI of the MI355X (gfx950) LiDAR motion-compensation library.
 *
 * This is the drop-in boundary for the reference's hot path.
 * The reference is pure Python, so the "FFI" a maintainer binds is ctypes:
 * every entry point takes plain pointers, sizes and ints, never a torch or
 * numpy type.  The Python host layer (livox-motion-compensation-sim_amd/)
 * mirrors the reference's own methods on top of these calls:
 *
 *   reference (file:line)                                      replaced by
 *   ---------------------------------------------------------  -----------------------------
 *   LiDARMotionSimulator.transform_pointcloud  LMC:772-776     mc_transform_pointcloud_f64 (one
 *                                                              call, host arrays, float64), or
 *                                                              mc_batch_upload_aos_f64 +
 *                                                              mc_deskew(MC_MODE_FRAME,
 *                                                              MC_POSE_DIRECT) +
 *                                                              mc_batch_download_aos_f64
 *   run_simulation pose selection + hot loop   LMC:802-832     mc_set_trajectory +
 *                                                              mc_batch_set_frame_times +
 *                                                              mc_deskew(MC_MODE_FRAME,
 *                                                              MC_POSE_SEARCHSORTED)
 *   save_results merge (np.vstack)             LMC:887-889     blocked-CSR batch layout;
 *                                                              mc_comm_gather_batch (multi-GPU)
 *   MotionCompensator.compensate_point_cloud   CSIM:1435-1480  mc_set_imu + mc_deskew_points_f64(MC_MODE_IMU)
 *                                                              (host float64 rows), or mc_deskew(MC_MODE_IMU)
 *                                                              on a device batch
 *     _interpolate_imu_data                    CSIM:1482-1516    (per-point gyro LERP in-kernel)
 *     _create_rotation_matrix                  CSIM:1518-1536    (R_xyz(theta)^T in-kernel)
 *   LiDARSimulator.simulate_scan / _raycast    CSIM:1011-1146  mc_set_ray_scene + mc_ray_count +
 *     (per frame of _simulate_lidar_frames     CSIM:2028-2084)   mc_ray_emit / mc_ray_emit_f64
 *   LivoxLVXWriter.write_lvx_file              CSIM:235-374    mc_csim_lvx_layout + mc_csim_lvx_encode /
 *     (lvx, lvx2, lvx3)                                          mc_csim_lvx_encode_batch
 *   DataExporter._export_pcd / _xyz / _csv     CSIM:1643-1715  mc_csim_text_encode / mc_csim_text_encode_batch
 *   (build-added)                          mc_deskew(MC_MODE_POSE_SLERP)
 *   (build-added: a11 into the sensor frame at a reference     mc_deskew_relative, mc_deskew_points_relative_f64,
 *    time per frame)                                             mc_pose_at, mc_batch_time_spans
 *
 * LMC = lidar_motion_compensation.py, CSIM = livox_mid70_complete_simulator.py.
 *
 * Conventions
 *  - Every function returns int: 0 = MC_OK, < 0 = error code; the message of the
 *    last failure on the calling thread is returned by mc_last_error().
 *  - The caller owns host buffers; a context owns device buffers; no host
 *    pointer is retained after a call returns.
 *  - All device work of a context is ordered on the context's own HIP stream.
 *    Calls that return host data synchronise that stream before returning;
 *    mc_deskew is asynchronous (mc_sync() waits for it).
 *  - One context per thread and device.
 *
 * Device layout of a batch ("blocked CSR"): n_frames ragged
 * frames; frame f holds count[f] points at padded indices [poff[f], poff[f]+count[f]);
 * poff[f] is a multiple of 256, so every frame starts on a block.  Block k holds
 * points 256k..256k+255 as C runs of 256 values: x, y, z, intensity (float32) and,
 * with MC_BATCH_WITH_TIME, t_ns (int32, nanoseconds since the frame start).
 */
#ifndef MCDESKEW_H_
#define MCDESKEW_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MC_ABI_VERSION 1

/* status codes */
#define MC_OK 0
#define MC_ERR_INVALID -1   /* bad argument / shape: Python maps to ValueError   */
#define MC_ERR_HIP -2       /* HIP runtime failure                                */
#define MC_ERR_NOMEM -3     /* device allocation failed                           */
#define MC_ERR_STATE -4     /* missing prerequisite (e.g. no trajectory uploaded) */
#define MC_ERR_INDEX -5     /* column count < 4: Python maps to IndexError (LMC:776) */
#define MC_ERR_COMM -6      /* RCCL failure                                       */
#define MC_ERR_SPACE -7     /* output buffer too small (the size needed is reported) */

/* deskew modes */
#define MC_MODE_FRAME 0      /* Path A: one SE(3) pose per frame, p' = R(rpy) p + t   (LMC:772-776)    */
#define MC_MODE_POSE_SLERP 1 /* per point: quaternion SLERP + position LERP of the pose table at
                                t_frame + t_ns*1e-9, then p' = R(q) p + pos       */
#define MC_MODE_IMU 2        /* Path B: per point gyro LERP, theta = w*dt, p' = R_xyz(theta)^T p
                                                                                 (CSIM:1435-1536) */

/* pose selection for MC_MODE_FRAME */
#define MC_POSE_SEARCHSORTED 0 /* idx = clamp(searchsorted(time, t_frame, 'left'), 0, T-1)  LMC:804-806 */
#define MC_POSE_DIRECT 1       /* frame f uses trajectory row f (explicit per-frame transformation)   */

/* batch creation flags */
#define MC_BATCH_WITH_TIME 1u  /* allocate the t_ns column (needed by SLERP / IMU modes) */
/* Keep the ASCII PCD text length (LMC:948) of every 256-point block beside the columns: the
 * kernels that write the batch's x|y|z|intensity (mc_deskew / mc_deskew_steps into it, the stager
 * mc_batch_upload_aos_f64 / mc_batch_stage_aos_f64_device, mc_scan_emit) also write those sums, so
 * mc_pcd_encode_batch skips its measure pass.  Any other write of the columns (column uploads,
 * synth, affine, gathers, mc_tune_order) marks the sums stale and the encoder measures again. */
#define MC_BATCH_WITH_PCD_LEN 2u

typedef struct mc_ctx mc_ctx;
typedef struct mc_batch mc_batch;
typedef struct mc_comm mc_comm;

/* ---- library / context ------------------------------------------------- */
int mc_abi_version(void);
const char* mc_last_error(void);
int mc_device_count(int* count);
/* PCI bus id ("dddd:bb:dd.f") of a visible device: tells ranks that share one GPU apart from
 * ranks on distinct GPUs (bench.py counts devices, not ranks) */
int mc_device_pci_bus_id(int device, char* out, int len);
int mc_create(int device, mc_ctx** out);
int mc_destroy(mc_ctx* ctx);
int mc_sync(mc_ctx* ctx);

/* ---- pose sources (copied to device; replace any previous table) ------- */
/* trajectory table of LMC:361-428: time (T,), position_gps (T,3), orientation_imu (T,3) rad,
 * all float64 C-contiguous.  time must be non-decreasing. */
int mc_set_trajectory(mc_ctx* ctx, int64_t n_poses, const double* time, const double* position,
                      const double* rpy);
/* IMU samples of CSIM:1191-1240: timestamp (M,) int64 ns, gyro (M,3) rad/s float64.
 * timestamps must be non-decreasing (duplicates allowed). */
int mc_set_imu(mc_ctx* ctx, int64_t n_samples, const int64_t* timestamp_ns, const double* gyro);

/* ---- batches ------------------------------------------------------------ */
int mc_batch_create(mc_ctx* ctx, int32_t n_frames, const int64_t* counts, uint32_t flags,
                    mc_batch** out);
int mc_batch_destroy(mc_batch* b);
int mc_batch_info(const mc_batch* b, int64_t* n_points, int64_t* padded_points, int32_t* n_frames,
                  int32_t* n_tiles);
/* padded frame offsets (n_frames+1 entries) as laid out on the device */
int mc_batch_padded_offsets(const mc_batch* b, int64_t* poff_out);
/* 1 when the batch's per-block PCD text sums describe its current columns (MC_BATCH_WITH_PCD_LEN
 * and the last write of the columns produced them), else 0 */
int mc_batch_pcd_len_current(const mc_batch* b, int32_t* current);
/* per-frame reference time in seconds (LMC:792-793 lidar_times) for SEARCHSORTED / SLERP */
int mc_batch_set_frame_times(mc_batch* b, const double* t_frame);
/* per-frame start timestamp in ns (CSIM:2049 frame['timestamp']) for MC_MODE_IMU */
int mc_batch_set_frame_start_ns(mc_batch* b, const int64_t* start_ns);

/* host dense AoS (N, ld) float64, columns 0..3 = x,y,z,intensity  ->  device SoA float32.
 * ld < 4 -> MC_ERR_INDEX (mirrors points[:, 3] in LMC:776). */
int mc_batch_upload_aos_f64(mc_batch* b, const double* aos, int64_t ld);
/* host dense columns (float32, N each); any pointer may be NULL to leave that column */
int mc_batch_upload_columns_f32(mc_batch* b, const float* x, const float* y, const float* z,
                                const float* intensity);
int mc_batch_upload_time_ns(mc_batch* b, const int32_t* t_ns);
/* device SoA float32 -> host dense AoS (N,4) float64 (the (N,4) f64 layout LMC:776 returns) */
int mc_batch_download_aos_f64(mc_batch* b, double* aos_out);
/* frames [f0, f1) only: (doff[f1] - doff[f0], 4) float64 rows (spot checks of batches too large
 * to bring back whole, e.g. BASELINE config 5's 1.2 G points) */
int mc_batch_download_frames_aos_f64(mc_batch* b, int32_t f0, int32_t f1, double* aos_out);
int mc_batch_download_columns_f32(mc_batch* b, float* x, float* y, float* z, float* intensity);
int mc_batch_download_time_ns(mc_batch* b, int32_t* t_ns);

/* ---- device buffers and the device-side stager ---------------------- */
/* The stager pair converts the reference's (N,4) float64 AoS (LMC:770 in, LMC:776 out) to and
 * from the batch's float32 SoA columns without leaving HBM; both are asynchronous on the ctx
 * stream and timed under mc_timing_read_layout. */
int mc_device_alloc(mc_ctx* ctx, int64_t bytes, void** dptr);
int mc_device_free(mc_ctx* ctx, void* dptr);
/* Device memory the library itself holds right now, over every context, batch and communicator of the
 * process: bytes and blocks (either may be NULL).  Back to what it was once the handles that
 * allocated are destroyed.  Not counted: the blocks mc_device_alloc hands to the caller, and pinned
 * host memory. */
int mc_device_memory_live(int64_t* bytes, int64_t* blocks);
int mc_memcpy_h2d(mc_ctx* ctx, void* dptr, const void* host, int64_t bytes);
int mc_memcpy_d2h(mc_ctx* ctx, void* host, const void* dptr, int64_t bytes);
int mc_memcpy_d2d(mc_ctx* ctx, void* dst, const void* src, int64_t bytes);
int mc_batch_stage_aos_f64_device(mc_batch* b, const double* d_aos, int64_t ld);
int mc_batch_fetch_aos_f64_device(mc_batch* b, double* d_aos);
int mc_timing_read_layout(mc_ctx* ctx, double* ms_total, int64_t* launches);

/* ---- scan_environment, the step before the path (LMC:701-770) ----------- */
/* scene points (n, ld>=4) float64 [x, y, z, intensity, ...], copied to the device */
int mc_set_environment(mc_ctx* ctx, int64_t n, const double* env, int64_t ld);
/* Pass 1 for F frames: sensor pose per frame from the trajectory (pose_select as mc_deskew's
 * frame mode; frame_times used by MC_POSE_SEARCHSORTED), visibility of every scene point,
 * params = {range_min, range_max, fov_horizontal, fov_vertical} (degrees, full angles),
 * systematic subsample to points_per_frame.  counts_out[F] = points each frame's scan keeps. */
int mc_scan_count(mc_ctx* ctx, int32_t n_frames, const double* frame_times, int pose_select,
                  const double* params, int64_t points_per_frame, int64_t* counts_out);
/* Pass 2: writes the scans into `out` (created with counts_out as frame counts) as sensor-frame
 * x,y,z + noise, intensity.  noise: (sum(counts), 3) float64 drawn by the caller in frame order
 * (LMC:767 np.random.normal), or NULL for noise-free scans. */
int mc_scan_emit(mc_ctx* ctx, mc_batch* out, const double* noise);
/* Pass 2 into the reference's own float64 arrays instead of a float32 batch: d_local receives every
 * frame's scan_environment output (LMC:770: sensor-frame x, y, z + noise, intensity) and d_aligned
 * (may be NULL) the frame loop's transform_pointcloud of it with the same pose (LMC:826-831), as
 * device (N, 4) float64 rows, frames back to back (N = sum of counts_out).  Bit-identical to the
 * reference's values: the pose's R is scipy's (mc_rotation_from_euler_xyz) and every product sum
 * accumulates as numpy's matmul does.  Synchronous. */
int mc_scan_emit_f64(mc_ctx* ctx, const double* noise, double* d_local, double* d_aligned);
int mc_timing_read_scan(mc_ctx* ctx, double* ms_total, int64_t* launches);

/* ---- LiDARSimulator.simulate_scan, the ray-march scanner behind Path B's frames (CSIM:1011-1146) -- */
/* The scene of _raycast (CSIM:1108-1146): n_objects point objects in list order, counts[o] rows each
 * (0 allowed: the reference skips empty objects, CSIM:1126), their rows (sum(counts), ld >= 4) float64
 * [x, y, z, intensity, ...] back to back; an object without an intensity column carries the
 * reference's 100 (CSIM:1140) in column 3.  Copied to the device; replaces any previous ray scene. */
int mc_set_ray_scene(mc_ctx* ctx, int32_t n_objects, const int64_t* counts, const double* rows, int64_t ld);
/* Pass 1 for F frames of n_rays rays each (simulate_scan's loop CSIM:1021-1031 over every frame of
 * _simulate_lidar_frames, CSIM:2037-2060, in one launch): origins (F, 3) sensor positions, R (F, 3, 3)
 * = R_z R_y R_x of the sensor orientation (CSIM:1105), dirs (n_rays, 3) the sensor-frame directions
 * (CSIM:1083-1086), steps[n_steps] = np.arange(range_min, range_max, step_size) (CSIM:1121) and
 * step_size, the march step and hit radius (CSIM:1118, 1131).  Every ray's first hit as the reference
 * decides it (first step with a point closer than step_size; first object in list order; closest
 * point, lowest index on ties).  counts_out[F] = hits per frame.  Synchronous. */
int mc_ray_count(mc_ctx* ctx, int32_t n_frames, const double* origins, const double* R, int32_t n_rays,
                 const double* dirs, int32_t n_steps, const double* steps, double step_size, int64_t* counts_out);
/* The last mc_ray_count's discrete result: hits_out (n_frames * n_rays, 3) int32 = step, object,
 * point index within the object (CSIM:1134-1135), or -1, -1, -1 for a miss. */
int mc_ray_hits(mc_ctx* ctx, int32_t* hits_out);
/* Pass 2 (CSIM:1033-1053): per hit, in frame and ray order, sensor_point = R_inv (hit_point -
 * position) with R_inv (F, 3, 3) = R_x(-roll) R_y(-pitch) R_z(-yaw) (CSIM:1170) plus noise, and the
 * hit's intensity plus noise clipped to [0, 255].  noise (sum(counts_out), 4) float64 = the three
 * range draws and the intensity draw of each hit (CSIM:1038-1039), or NULL for none.  mc_ray_emit
 * writes a batch created with counts_out as frame counts: float32 x, y, z, intensity and, with
 * MC_BATCH_WITH_TIME, t_ns = 1000 * ray index (CSIM:1048).  mc_ray_emit_f64 writes host rows
 * (sum(counts_out), 5) float64 = x, y, z, intensity (not yet truncated by int(), CSIM:1047), ray
 * index.  MC_ERR_STATE when the ray scene changed since the count.  Synchronous. */
int mc_ray_emit(mc_ctx* ctx, mc_batch* out, const double* R_inv, const double* noise);
int mc_ray_emit_f64(mc_ctx* ctx, const double* R_inv, const double* noise, double* rows_out);
int mc_timing_read_ray(mc_ctx* ctx, double* ms_total, int64_t* launches);

/* ---- output codecs, encoded from a device (N, ld) float64 AoS cloud whose
 * frames lie back to back (counts[f] rows each): the array layout the reference hands its writers.
 * Both are synchronous and timed under mc_timing_read_codec. ------------------------------------ */
/* LVX v1.1 layout (LMC:113-132): byte offset of every frame; frame_pos[F] = file size. Host only. */
int mc_lvx_layout(int32_t n_frames, const int64_t* counts, int64_t* frame_pos);
/* The whole LVX v1.1 file of LivoxLVXWriter.write_compatible_lvx (LMC:57-272) into d_out
 * (>= frame_pos[F] bytes, 2-byte aligned): 88-byte file header, per frame a 24-byte header
 * (offset, next offset, frame_ids[f]) and 96-point packages stamped timestamp_ns[f]
 * (= int(timestamp * 1e9), LMC:176).  ld >= 3; has_intensity[f] == 0 gives reflectivity 128
 * (LMC:268); has_intensity NULL means (ld > 3).  A NaN coordinate or intensity -> MC_ERR_INVALID
 * (the reference's int(nan) fails its write). */
int mc_lvx_encode(mc_ctx* ctx, const double* d_aos, int64_t ld, int32_t n_frames, const int64_t* counts,
                  const uint64_t* frame_ids, const uint64_t* timestamp_ns, const uint8_t* has_intensity,
                  void* d_out, int64_t out_bytes);
/* ASCII PCD point lines of save_pcd (LMC:946-948, "%.6f %.6f %.6f %.6f\n", Python's correctly
 * rounded formatting) for F clouds, back to back in d_out; body_pos[F+1] receives each cloud's byte
 * offset (body_pos[F] = total).  If out_bytes < total: MC_ERR_SPACE, body_pos filled, nothing
 * written.  |value| >= 2^107 -> MC_ERR_INVALID (beyond the device formatter). */
int mc_pcd_encode(mc_ctx* ctx, const double* d_aos, int64_t ld, int32_t n_frames, const int64_t* counts,
                  void* d_out, int64_t out_bytes, int64_t* body_pos);
/* The same two encoders reading a batch's own float32 columns in HBM (frames = the batch's frames,
 * 4 columns, intensity present): the bytes mc_lvx_encode / mc_pcd_encode produce from the batch's
 * values widened to float64 (mc_batch_fetch_aos_f64_device), without that 48 B/point pass and
 * with 16 instead of 32 B/point read.  The writers behind save_results (LMC:887-921) and the
 * LVX export (LMC:24-272) on a device-resident, deskewed batch. */
int mc_lvx_encode_batch(mc_ctx* ctx, const mc_batch* b, const uint64_t* frame_ids, const uint64_t* timestamp_ns,
                        void* d_out, int64_t out_bytes);
int mc_pcd_encode_batch(mc_ctx* ctx, const mc_batch* b, void* d_out, int64_t out_bytes, int64_t* body_pos);
/* Deskew -> ASCII PCD in one call: mc_deskew(in -> out) (out != in), whose kernel also sums each
 * output block's text bytes, then the PCD lines of out as mc_pcd_encode_batch writes them, with no
 * separate measure pass over out (the reference's LMC:831 -> 887-889 -> 932-948 sequence on
 * device-resident frames; a block holding a value beyond the packed formatter, |v| >= 4294 / NaN /
 * inf, falls back to the measure pass).  MC_ERR_SPACE as mc_pcd_encode_batch: out is deskewed and
 * body_pos filled, no text written.  The deskew kernel is timed under mc_timing_read, the writer
 * under mc_timing_read_codec. */
int mc_deskew_pcd(mc_ctx* ctx, const mc_batch* in, mc_batch* out, int mode, int pose_select, void* d_out,
                  int64_t out_bytes, int64_t* body_pos);
int mc_timing_read_codec(mc_ctx* ctx, double* ms_total, int64_t* launches);

/* ---- CSIM exports: LivoxLVXWriter.write_lvx_file (CSIM:235-374) and DataExporter's PCD / XYZ / CSV
 * (CSIM:1603-1715), byte-identical.  Source: device rows (N, ld >= 5) float64 = x, y, z, intensity,
 * timestamp (the points_array of CSIM:1627) with frames back to back, or a MC_BATCH_WITH_TIME batch
 * whose frame starts are set; the row of a batch point is defined as [x, y, z, trunc(intensity),
 * frame_start_ns[f] + t_ns] with the float32 values widened exactly (the LiDARPoint of CSIM:1040-1050),
 * so the *_batch encoders give the bytes of the row encoders applied to those rows.  ld < 5 ->
 * MC_ERR_INDEX; a batch without time or frame starts -> MC_ERR_STATE.  Synchronous; timed under
 * mc_timing_read_codec. ------------------------------------------------------------------------- */
#define MC_CSIM_LVX_LEGACY 1 /* "lvx":  _write_lvx_legacy, float32 records            CSIM:256-267, 295-321 */
#define MC_CSIM_LVX2 2       /* "lvx2": _write_lvx2, int32 mm records                 CSIM:269-287, 323-374 */
#define MC_CSIM_LVX3 3       /* "lvx3": the bytes of lvx2                             CSIM:289-293          */
#define MC_CSIM_PCD 0        /* _export_pcd body "%.6f %.6f %.6f %.0f %.0f\n"         CSIM:1663-1664        */
#define MC_CSIM_XYZ 1        /* _export_xyz "%.6f %.6f %.6f\n" (np.savetxt)           CSIM:1700-1706        */
#define MC_CSIM_CSV 2        /* _export_csv rows "%.6f,%.6f,%.6f,%.6f,%.6f\n", NaN = empty field  CSIM:1708-1715 */
/* File layout (CSIM:269-374): lvx2 / lvx3 = 88 header bytes, then per frame 45 + 14 n bytes (24-byte
 * frame header, the 21-byte package header the code writes, n records); legacy = 60 header bytes,
 * then 12 + 14 n per frame.  frame_pos[F] = file size.  Host only. */
int mc_csim_lvx_layout(int version, int32_t n_frames, const int64_t* counts, int64_t* frame_pos);
/* The whole file of write_lvx_file (CSIM:245-374) into d_out (>= frame_pos[F] bytes, else
 * MC_ERR_SPACE): headers from lidar_sn (16 bytes, ASCII padded with zeros), device_type,
 * extrinsic_enable and extrinsics[6] = roll, pitch, yaw, x, y, z (CSIM:302-306, 323-341); frame f
 * stamped timestamp_ns[f] (frame['timestamp']) and, in lvx2, numbered f (CSIM:286).  Records: lvx2
 * int(v * 1000) without a clip (CSIM:368-372), legacy float32 (CSIM:319), then trunc(intensity) and
 * d_tags[row] (N bytes on the device; NULL = 0).  Where the reference's write raises — lvx2: a NaN or
 * infinite coordinate, int(v * 1000) outside int32; legacy: a finite coordinate that rounds to +-inf in
 * float32; both: an intensity that is NaN or outside 0..255 after truncation — MC_ERR_INVALID, and
 * the contents of d_out are unspecified. */
int mc_csim_lvx_encode(mc_ctx* ctx, int version, const double* d_rows, int64_t ld, int32_t n_frames,
                       const int64_t* counts, const uint64_t* timestamp_ns, const uint8_t* d_tags,
                       const uint8_t* lidar_sn, uint8_t device_type, uint8_t extrinsic_enable,
                       const float* extrinsics, void* d_out, int64_t out_bytes);
int mc_csim_lvx_encode_batch(mc_ctx* ctx, int version, const mc_batch* b, const uint64_t* timestamp_ns,
                             const uint8_t* d_tags, const uint8_t* lidar_sn, uint8_t device_type,
                             uint8_t extrinsic_enable, const float* extrinsics, void* d_out, int64_t out_bytes);
/* The point lines of DataExporter._export_pcd / _export_xyz / _export_csv (CSIM:1643-1715) for F
 * clouds, back to back in d_out; the PCD header (CSIM:1648-1659) and the CSV header line are the
 * host's.  "%.6f" and "%.0f" are Python's correctly rounded formatting ("%.0f": ties to even on the
 * exact binary value, "-0" for a negative value that rounds to zero, nan / inf / -inf); MC_CSIM_CSV
 * prints a NaN as an empty field.  The mc_pcd_encode contract: body_pos[F+1] receives each cloud's
 * byte offset (body_pos[F] = total); if out_bytes < total: MC_ERR_SPACE, body_pos filled, nothing
 * written.  |value| >= 2^107 -> MC_ERR_INVALID. */
int mc_csim_text_encode(mc_ctx* ctx, int format, const double* d_rows, int64_t ld, int32_t n_frames,
                        const int64_t* counts, void* d_out, int64_t out_bytes, int64_t* body_pos);
int mc_csim_text_encode_batch(mc_ctx* ctx, int format, const mc_batch* b, void* d_out, int64_t out_bytes,
                              int64_t* body_pos);

/* ---- ingest (f7): the inverse of the writers above -------------------------------------------
 * Recorded LVX files and ASCII PCD / XYZ / CSV text decoded on the device into float64 rows
 * [x, y, z, intensity, timestamp_ns] (the points_array of CSIM:1627) plus one tag byte per point, or
 * into the float32 columns of a batch ("float64, rounded once").  The layout is sniffed from the
 * bytes: MC_LVX_V11 (what mc_lvx_encode writes, LMC:57-272), MC_CSIM_LVX_LEGACY (CSIM:256-267,
 * 295-321) and MC_CSIM_LVX2 (CSIM:269-293, 323-374; an lvx3 file is the same bytes and reports lvx2).
 *   int32 mm records   x = float64(mm) / 1000.0, one IEEE division       (inverse of LMC:257, CSIM:368)
 *   legacy records     the float32 widened exactly                        (inverse of CSIM:319)
 *   intensity          V11: reflectivity / 255.0 (LMC:266); CSIM: the byte 0..255 (CSIM:320, 373)
 *   timestamp          the frame's (V11: the package's, LMC:237) + point_period_ns * (index in frame),
 *                      added in int64, then converted to float64
 * What the files do not hold: (1) NONE OF THESE FORMATS STORES A PER-POINT TIME — point_period_ns
 * (default 0) is the caller's knowledge; (2) V11 stores no point count and pads a frame's last package
 * with zero records (LMC:246-250): by default the trailing all-zero records of each frame's last package
 * are dropped (counted on the device), so a trailing real point at the origin with reflectivity 0 is
 * dropped too; keep_padding keeps every slot (96 x packages).  A V11 frame without a package has no
 * timestamp: -1.  Re-encoding decoded mm records need not reproduce the file: both writers truncate
 * x * 1000, and (m / 1000.0) * 1000 can fall just below m; legacy files and the text formats round-trip.
 *
 * mc_lvx_probe / mc_lvx_index are host only and validate everything a launch relies on: magic and
 * version, offsets increasing and inside the file, (frame size - 24) % 1366 == 0 for V11, position +
 * header + 14 * count <= bytes for the CSIM layouts.  A file that fails -> MC_ERR_INVALID with a
 * message, nothing launched.  The decoders re-check frame_pos / counts against `bytes` and never
 * follow an offset stored in the file.  d_file / d_text: device copies of the file, 16-byte aligned
 * and allocated up to the next multiple of 16 bytes (the kernels load whole 16-byte chunks).
 * frame_pos[F + 1]: each frame header's offset, then the file size; slots[F]: record slots per frame.
 * frame_ids: V11 the stored id, lvx2 the stored index, legacy the position.  Any output may be NULL. */
#define MC_LVX_V11 0
int mc_lvx_probe(const void* file, int64_t bytes, int* format, int32_t* n_frames);
int mc_lvx_index(const void* file, int64_t bytes, int format, int32_t n_frames, int64_t* frame_pos, int64_t* slots,
                 uint64_t* frame_ids, int64_t* timestamp_ns, uint8_t* lidar_sn16, uint8_t* device_type,
                 uint8_t* extrinsic_enable, float* extrinsics6);
/* counts_out[F]: the points per frame — slots for the CSIM layouts and with keep_padding, else V11's
 * slots less the trailing zero records of each frame's last package (k_lvx_trim). */
int mc_lvx_count(mc_ctx* ctx, int format, const void* d_file, int64_t bytes, int32_t n_frames,
                 const int64_t* frame_pos, const int64_t* slots, int keep_padding, int64_t* counts_out);
/* d_rows (sum(counts), ld >= 5) float64, frames back to back; d_tags [sum(counts)] or NULL.  ld < 5 ->
 * MC_ERR_INDEX.  timestamp_ns[F]: the frame timestamps of mc_lvx_index (V11 reads its package headers
 * and takes NULL).  Synchronous; timed under mc_timing_read_codec. */
int mc_lvx_decode(mc_ctx* ctx, int format, const void* d_file, int64_t bytes, int32_t n_frames,
                  const int64_t* frame_pos, const int64_t* counts, const int64_t* timestamp_ns,
                  int64_t point_period_ns, double* d_rows, int64_t ld, uint8_t* d_tags);
/* The same into a batch created with MC_BATCH_WITH_TIME (else MC_ERR_STATE) whose counts equal
 * `counts`: columns = float32 of the row values, t_ns = index * point_period_ns (must fit int32, else
 * MC_ERR_INVALID before any launch), frame starts = timestamp_ns. */
int mc_lvx_decode_batch(mc_ctx* ctx, int format, const void* d_file, int64_t bytes, int32_t n_frames,
                        const int64_t* frame_pos, const int64_t* counts, const int64_t* timestamp_ns,
                        int64_t point_period_ns, mc_batch* out, uint8_t* d_tags);
/* ASCII point lines: LMC save_pcd (4 fields, LMC:932-948), CSIM _export_pcd (5 fields, CSIM:1648-1664),
 * _export_xyz (3 fields, CSIM:1700-1706), _export_csv (5 comma-separated fields, an empty field = NaN,
 * CSIM:1708-1715); the host strips the PCD header / CSV header line and passes the body.  sep ' ' or
 * ','; n_cols 3..8.  A line holding nothing or a lone '\r' is skipped, a trailing '\r' ignored, the
 * last line may lack its '\n'.  Tokens: [+-]digits[.digits], nan, inf, -inf.  With the sign, leading
 * zeros and the fraction's trailing zeros stripped, a token of at most 19 significant digits and at
 * most 19 fractional digits decodes bit-equal to strtod / Python float(); anything else (an exponent,
 * more digits, other text) is beyond the device parser: MC_ERR_INVALID with *bad_line = the first such
 * line (1-based among the non-empty lines) — no host fallback, as the formatters' |v| >= 2^107.  A
 * line with another number of fields: the same.  mc_text_decode: n_lines must be mc_text_lines' count;
 * ld < n_cols -> MC_ERR_INDEX.  mc_text_decode_batch: the batch's points must equal the line count
 * (frames = its counts); x, y, z, intensity = float32(float64(token)) (3 columns: intensity 0); with
 * n_cols >= 5 the batch needs MC_BATCH_WITH_TIME (else MC_ERR_STATE) and t_ns = int64(column 4) -
 * frame_start_ns[f] (NULL: the frame's first point's timestamp; frame_start_out[F], may be NULL,
 * receives the starts used), which must fit int32 (else MC_ERR_INVALID).  Synchronous. */
int mc_text_lines(mc_ctx* ctx, const void* d_text, int64_t bytes, int64_t* n_lines);
int mc_text_decode(mc_ctx* ctx, int sep, int32_t n_cols, const void* d_text, int64_t bytes, int64_t n_lines,
                   double* d_rows, int64_t ld, int64_t* bad_line);
int mc_text_decode_batch(mc_ctx* ctx, int sep, int32_t n_cols, const void* d_text, int64_t bytes, mc_batch* out,
                         const int64_t* frame_start_ns, int64_t* frame_start_out, int64_t* bad_line);

/* ---- LAS 1.2 (f8): the files of save_las (LMC:950-963) and _export_las (CSIM:1671-1698), both thin
 * laspy calls in the reference, written and read on the device without laspy.  Little-endian, a
 * 227-byte public header block, no VLRs on write, point formats 0..3 (20 / 28 / 26 / 34-byte records:
 * X, Y, Z i32, intensity u16, six zero bytes, [gps_time f64], [R, G, B u16 = 0]).
 *   X = int32(rint((x - offset) / scale)): subtract, IEEE divide, round half to even (np.round);
 *   intensity = trunc(column 3 * intensity_mul) as u16; gps_time = time * time_mul in float64
 *   (time_mul == 0: 0.0).  LMC:950-963 is intensity_mul 65535, time_mul 0; CSIM:1671-1698 is
 *   intensity_mul 1, time_mul 1e-9, scale 0.001.  Every other record byte is 0 (return number 0
 *   included) and the points-by-return counts are 0, as the reference leaves them.  Header bounds =
 *   min / max of the stored integers * scale + offset (host, float64, multiply then add); system
 *   identifier "OTHER"; 0.0 bounds for an empty cloud.
 * NOT CLAIMED: laspy is not available where this was written, so no file of its making was compared.
 * Byte equality with laspy's own header choices (identifier strings, creation date, by-return counts)
 * is neither promised nor tested, and the 0.01 scale the Python layer defaults to for the LMC variant
 * is laspy's documented default from memory, unchecked.  Scale and offset are parameters, so any
 * other writer can be matched.
 * Refused (MC_ERR_INVALID naming the first such row, *bad_row = that row, may be NULL; where numpy
 * wraps around silently): a coordinate that is not finite, rint(...) outside int32, an intensity that
 * is NaN or outside 0..65535 after truncation, n >= 2^32.  Too small a buffer -> MC_ERR_SPACE with
 * the size needed (227 + n * record bytes) in the message.  Synchronous; timed under
 * mc_timing_read_codec. ------------------------------------------------------------------------- */
/* Host only: parse an untrusted header (file = the first bytes .. the whole file, bytes = the file
 * size).  Accepted: "LASF", version 1.0 .. 1.3, formats 0..3, header size >= 227, offset to point
 * data >= header size, record length >= the format's nominal size, offset + n * record length <=
 * bytes; everything else MC_ERR_INVALID with a message, nothing reported.  bounds[6] = max x, min x,
 * max y, min y, max z, min z as stored.  Any output may be NULL.  (LMC:950-963 / CSIM:1671-1698) */
int mc_las_probe(const void* file, int64_t bytes, int32_t* point_format, int32_t* record_length,
                 int64_t* offset_to_points, int64_t* n_points, double* scale, double* offset, double* bounds);
/* The whole file into d_out from device rows (n, ld) float64 = x, y, z, intensity[, time]
 * (ld >= 4, >= 5 when time_mul != 0, else MC_ERR_INDEX).  scale[3] finite > 0, offset[3] finite;
 * software: the generating-software field (at most 32 bytes, NULL = "mcdeskew"); year / day_of_year:
 * the creation date.  (LMC:950-963 / CSIM:1671-1698) */
int mc_las_encode(mc_ctx* ctx, const double* d_rows, int64_t ld, int64_t n, int point_format, const double* scale,
                  const double* offset, double intensity_mul, double time_mul, const char* software, int32_t year,
                  int32_t day_of_year, void* d_out, int64_t out_bytes, int64_t* bad_row);
/* The same from a batch's float32 columns, widened exactly to float64 and run through the same
 * formula, points in dense order; time = frame_start_ns[f] + t_ns, converted to float64, then
 * multiplied (time_mul != 0 needs MC_BATCH_WITH_TIME and the frame starts, else MC_ERR_STATE).
 * (LMC:950-963 / CSIM:1671-1698) */
int mc_las_encode_batch(mc_ctx* ctx, const mc_batch* batch, int point_format, const double* scale,
                        const double* offset, double intensity_mul, double time_mul, const char* software,
                        int32_t year, int32_t day_of_year, void* d_out, int64_t out_bytes, int64_t* bad_row);
/* Decode the records of a file whose header mc_las_probe accepted (the numbers are re-checked against
 * `bytes`; no kernel follows a number stored in the file): d_file = the device copy of the file,
 * 16-byte aligned and allocated up to a multiple of 16 bytes; any offset_to_points >= 227, any
 * record_length >= nominal (extra bytes skipped).  d_rows (n, ld >= 5) float64 = x, y, z, intensity,
 * gps_time in seconds (0.0 for formats 0 and 2); x = X * scale + offset as a float64 multiply, rounded,
 * then an add, rounded (never fused).  (LMC:950-963 / CSIM:1671-1698) */
int mc_las_decode(mc_ctx* ctx, const void* d_file, int64_t bytes, int point_format, int64_t record_length,
                  int64_t offset_to_points, int64_t n_points, const double* scale, const double* offset,
                  double* d_rows, int64_t ld);
/* The same into a MC_BATCH_WITH_TIME batch of n_points points (frames = its counts): x, y, z =
 * float32 of the float64 values, intensity = float32(intensity * intensity_scale), t_ns =
 * int64(rint(gps_time * 1e9)) - frame_start_ns[f] (NULL: each frame's first point's time;
 * frame_start_out[F], may be NULL, receives the starts used), which must fit int32, else
 * MC_ERR_INVALID naming the first such point (*bad_row).  (LMC:950-963 / CSIM:1671-1698) */
int mc_las_decode_batch(mc_ctx* ctx, const void* d_file, int64_t bytes, int point_format, int64_t record_length,
                        int64_t offset_to_points, int64_t n_points, const double* scale, const double* offset,
                        double intensity_scale, mc_batch* out, const int64_t* frame_start_ns,
                        int64_t* frame_start_out, int64_t* bad_row);

/* ---- voxel-grid downsampling (build-added; csrc/voxel_core.hpp, voxel.hpp) ---------------------
 * One output point per occupied voxel of a grid of size `voxel` anchored at `origin`: the mean of
 * the voxel's points, with integer per-voxel sums, so the result is the same bit for bit on every
 * run whatever order the device's atomics arrive in.  Per point and axis, every line ONE IEEE float64
 * operation (no contraction):
 *   a = double(v) - o     g = a / h     k = floor(g)     f = g - k        (f may round up to 1.0)
 *   Q  = (int64) rint(f * 2^32),  0 <= Q <= 2^32;      QI = (int64) rint(double(intensity) * 2^16)
 * A voxel is one (kx, ky, kz); its record is n, S[3] = sum Q, SI = sum QI (int64).  Per voxel:
 *   m = double(S) / double(n)     w = double(k) + m * 2^-32     c = o + w * h
 *   i = (double(SI) / double(n)) * 2^-16
 * Voxels come out in order of first appearance (voxel A before B when A's lowest-index point is
 * before B's; a batch's index order is frame-major, then the index within the frame; padding slots
 * are not points).
 * Accuracy, a property of the definition (checked on the CPU against exact rational means):
 * |c - mean| <= h * 2^-32 plus the float64 rounding of the operations above (half an ulp each of a,
 * g, w, w * h and c).  For h in 0.01 .. 0.5 and keys up to +-1 048 575 the worst seen at origin 0 is
 * 1.1e-10 h; at an origin of 5e6 m half an ulp of c itself (4.7e-10 m) is the larger part.  The
 * float32 batch output is within 1 float32 ulp of the correctly rounded mean; the intensity is within
 * 2^-17 of the mean (reached).
 * Refused: a coordinate or its g not finite, a k outside [-2^20, 2^20), an intensity not finite or
 * with |intensity| > 65536.  One refused point fails the whole build with MC_ERR_INVALID naming the
 * lowest one (*bad_frame / *bad_index, or *bad_row; -1 when none) and leaves nothing to emit.
 * Count-then-emit, as mc_scan_count / mc_scan_emit: a build completes the sums and reports
 * *n_voxels = M, so the emits need the source no more and may be called repeatedly.  An emit
 * without a successful build: MC_ERR_STATE.  voxel <= 0 or not finite, origin not finite, ld < 4,
 * 2^31 points or more: MC_ERR_INVALID.
 * Device memory, the context's, kept (and reused while large enough) until mc_destroy, or until
 * mc_voxel_release, which frees it early (optional; MC_OK when there is nothing): 16 B per table slot (the power of two >= 2 N slots, so 32 .. 64 B per
 * point), 8 B + 1/8 B per point, 36 B per voxel — 2.1 GB + 0.5 GB + up to 2.2 GB for 60 M points.  The
 * emits allocate nothing. */
int mc_voxel_build_batch(mc_ctx* ctx, const mc_batch* in, double voxel, const double* origin, int64_t* n_voxels,
                         int32_t* bad_frame, int64_t* bad_index);
/* d_rows: device (n, ld) float64 rows x, y, z, intensity, ... */
int mc_voxel_build_f64(mc_ctx* ctx, const double* d_rows, int64_t ld, int64_t n, double voxel, const double* origin,
                       int64_t* n_voxels, int64_t* bad_row);
/* out: a batch of one frame of exactly M points (else MC_ERR_INVALID); receives float(c), float(i);
 * a time column is left alone; MC_BATCH_WITH_PCD_LEN sums are marked stale. */
int mc_voxel_emit_batch(mc_ctx* ctx, mc_batch* out);
/* device outputs, any may be NULL: d_rows (M, 4) float64 cx, cy, cz, i (16-byte aligned); d_counts
 * (M,) int32 points per voxel; d_keys (M, 3) int32 */
int mc_voxel_emit_f64(mc_ctx* ctx, double* d_rows, int32_t* d_counts, int32_t* d_keys);
/* event time (ms) of the timed phases since the last read: ms_phase[4] = insert (with the table
 * reset), rank, accumulate, finalise; *launches = timed regions */
int mc_timing_read_voxel(mc_ctx* ctx, double* ms_phase, int64_t* launches);
int mc_voxel_release(mc_ctx* ctx);

/* ---- growing a voxel cloud: inserting points and merging exact sums --------------------------------
 * The definition: after any sequence of mc_voxel_insert_* / mc_voxel_merge_sums calls on a live build, the
 * cloud is BIT FOR BIT the cloud mc_voxel_build_* returns for the concatenation of the sources in call
 * order.  The per-voxel record is integer, so adding records is exact and independent of order, and
 * voxels are numbered by first appearance, so later voxels follow earlier ones.
 * An item is a point, or a voxel record (key, n, S[3], SI) that stands for n points of that voxel
 * arriving together.  Items are indexed in source order: frame-major, then the index within the frame,
 * for a batch (padding slots are not points); the row for rows; the record index for records.  For a
 * call on a cloud of M voxels and N points:
 *   1. every item is quantised, or checked, with the cloud's own voxel size and origin (no grid arguments)
 *   2. an item whose key the cloud holds adds into that voxel's record; a voxel's id never changes:
 *      ids 0 .. M-1 keep their keys and their order
 *   3. keys new to the cloud become voxels M, M+1, ... in order of the lowest item index that holds them
 *      (a key may occur in any number of records of one merge); *n_new is their number
 *   4. N grows by the points of the call (the sum of n for records).  A call that would make N >= 2^31 is
 *      refused: the uint32 count, the int32 emit and |S| < 2^63 stay safe
 *   5. a refused call changes nothing: a point the build refuses, a record with n < 1, a key outside
 *      [-2^20, 2^20), S[c] outside 0 .. n * 2^32 or |SI| > n * 2^32, or the 2^31 limit is MC_ERR_INVALID,
 *      naming the lowest refused item (*bad_frame / *bad_index, *bad_row, *bad_record; -1 when none, as
 *      for the limit); afterwards the cloud is live and every emit is bit-equal to what it was.  (A failure that
 *      is no refusal, MC_ERR_NOMEM or MC_ERR_HIP once the table has been touched, leaves no live build.)
 *   6. the centroids, normals and clustering derived from the cloud are invalidated as by a new build:
 *      the next analysis sees the grown cloud
 * The build of an empty source (n = 0) is a valid target: the way to start a map from nothing.  An empty
 * call is MC_OK and changes nothing.  Without a live build: MC_ERR_STATE.  The cost is that of the call's
 * items (one pass that validates, one that inserts, the rank scan, one that accumulates; two
 * synchronisations), apart from growth: the table stays at most half full for the worst case of every
 * item bringing a new key, so M + items > slots / 2 makes a table of the power of two >= 2 (M + items)
 * slots and re-inserts the M keys; the per-voxel records grow geometrically, their contents copied.
 * Outputs never depend on the table's size. */
int mc_voxel_insert_batch(mc_ctx* ctx, const mc_batch* in, int64_t* n_new, int32_t* bad_frame, int64_t* bad_index);
/* d_rows: device (n, ld) float64 rows x, y, z, intensity, ...; the definition above */
int mc_voxel_insert_f64(mc_ctx* ctx, const double* d_rows, int64_t ld, int64_t n, int64_t* n_new, int64_t* bad_row);
/* The raw sums of the live build, queued: d_sums (M, 4) int64 Sx, Sy, Sz, SI in the cloud's order.  With the
 * d_keys and d_counts of mc_voxel_emit_f64 they are the cloud's records: what mc_voxel_merge_sums takes, and by
 * the definition above merging them into a cloud of the same grid equals inserting the points they stand for. */
int mc_voxel_emit_sums(mc_ctx* ctx, int64_t* d_sums);
/* m records as items (the definition above): device d_keys (m, 3) int32, d_counts (m,) int32, d_sums (m, 4)
 * int64.  The records must come from the cloud's own grid (voxel size and origin, bit for bit): the caller's
 * to check, the keys carry no grid. */
int mc_voxel_merge_sums(mc_ctx* ctx, const int32_t* d_keys, const int32_t* d_counts, const int64_t* d_sums, int64_t m,
                        int64_t* n_new, int64_t* bad_record);
/* N of the definition above: the points the live build holds.  Host state; needs no synchronisation. */
int mc_voxel_points(mc_ctx* ctx, int64_t* n_points);
/* For tests of the growth rule (either may be NULL): the slots of the live build's table (0: the build of an
 * empty source has none yet) and the times an insert or a merge has made a new table since the build. */
int mc_voxel_table(mc_ctx* ctx, int64_t* slots, int64_t* growths);
/* event time (ms) of the phases of the inserts and merges since the last read: ms_phase[4] = validate,
 * insert (with the table's growth), rank, accumulate; *launches = timed regions */
int mc_timing_read_voxel_insert(mc_ctx* ctx, double* ms_phase, int64_t* launches);

/* ---- shrinking a voxel cloud: removing voxels and subtracting exact sums -----------------------------
 * The way out of the live build, as exact as the way in: the records are integers, so a subtraction undoes
 * an addition bit for bit.
 * mc_voxel_remove: d_mask is device (M,) bytes; the voxels whose byte is not 0 leave.  The survivors keep
 * their relative order and get ids 0 .. M' - 1; *n_removed = M - M'.  Afterwards the cloud is BIT FOR BIT,
 * in every emit and in N, the cloud mc_voxel_build_* returns for the concatenated sources with the points
 * of the removed voxels left out (removing whole voxels changes no other voxel's first appearance).
 * mc_voxel_subtract_*: the items of mc_voxel_insert_* / mc_voxel_merge_sums, leaving.  For a call on a
 * cloud of M voxels and N points:
 *   1. every item is quantised, or checked, with the cloud's own voxel size and origin, as an insert's
 *   2. its Q[3], QI and n (1 for a point) are subtracted from the record of its voxel
 *   3. a voxel whose count reaches 0 leaves as in mc_voxel_remove; *n_emptied is their number
 *   4. N falls by the points of the call
 *   5. insert then subtract of the same source, or merge then subtract of the same records, is the
 *      identity in every emit, whatever voxels the source shares with the cloud; for the build of A
 *      followed by B, subtracting A leaves exactly the records of the build of B, in the relative order
 *      they had (a build of B alone may number them differently: a voxel's first point may have been A's)
 *   6. a refused call changes nothing and is MC_ERR_INVALID with *why saying which of these it was:
 *        MC_VOXEL_SUB_ITEM       an item an insert or a merge refuses
 *        MC_VOXEL_SUB_MISSING    an item whose voxel the cloud does not hold
 *        MC_VOXEL_SUB_POINTS     the call brings more points than the cloud holds (no item is named)
 *        MC_VOXEL_SUB_REMAINDER  a voxel would be left with a record that no set of points sums to: a
 *                                count below 0, a count of 0 with a sum that is not 0, or a count n' >= 1
 *                                with a coordinate sum outside 0 .. n' * 2^32 or |SI| > n' * 2^32
 *      The lowest refused item is named (*bad_frame / *bad_index, *bad_row, *bad_record; -1 when none);
 *      for the last kind it is the lowest item whose voxel ended up invalid, and the message holds that
 *      voxel's key.  ITEM and MISSING are found together, before anything is written: the lower item of
 *      either kind is named.  (A failure that is no refusal, once the records have been touched, leaves no
 *      live build.)
 *   7. the cloud cannot know whether the subtracted points were ever inserted: that a record which passes
 *      these checks is the record of the points meant to stay is the caller's contract
 *   8. the centroids, normals and clustering derived from the cloud are invalidated as by an insert
 * An empty call, or a mask without a set byte, is MC_OK and touches nothing.  Removing every voxel leaves
 * an empty live cloud that an insert fills again.  Without a live build: MC_ERR_STATE.
 * Cost.  A subtraction that empties no voxel costs what its items cost (one pass that validates and looks
 * the keys up, read-only; one that subtracts; one that checks; two synchronisations): no pass over the
 * table or the cloud.  A removal, and a subtraction that empties a voxel, cost what the CLOUD costs, not
 * what leaves: the keep flags and their scan, one pass that moves the survivors' records into fresh arrays
 * (swapped afterwards), and the table cleared and refilled from the survivors' keys.  The table keeps its
 * size unless the survivors fill less than an eighth of it; then it shrinks to the power of two >= 4 M',
 * at least 64 slots (mc_voxel_table reports it; a shrink is no growth).  Not built: tombstones, which
 * would make a removal cost what leaves but put a compare into every probe loop of the build, the insert
 * and the window walks; subtracting one frame of a batch; normals kept across a removal. */
#define MC_VOXEL_SUB_OK 0
#define MC_VOXEL_SUB_ITEM 1
#define MC_VOXEL_SUB_MISSING 2
#define MC_VOXEL_SUB_POINTS 3
#define MC_VOXEL_SUB_REMAINDER 4
int mc_voxel_remove(mc_ctx* ctx, const uint8_t* d_mask, int64_t* n_removed);
/* the arguments of mc_voxel_insert_batch, *n_emptied for *n_new, and *why (may be NULL) */
int mc_voxel_subtract_batch(mc_ctx* ctx, const mc_batch* in, int64_t* n_emptied, int32_t* bad_frame, int64_t* bad_index,
                            int32_t* why);
/* the arguments of mc_voxel_insert_f64, *n_emptied for *n_new, and *why (may be NULL) */
int mc_voxel_subtract_f64(mc_ctx* ctx, const double* d_rows, int64_t ld, int64_t n, int64_t* n_emptied, int64_t* bad_row,
                          int32_t* why);
/* the arguments of mc_voxel_merge_sums, *n_emptied for *n_new, and *why (may be NULL): every record stands for
 * its n points leaving together */
int mc_voxel_subtract_sums(mc_ctx* ctx, const int32_t* d_keys, const int32_t* d_counts, const int64_t* d_sums, int64_t m,
                           int64_t* n_emptied, int64_t* bad_record, int32_t* why);
/* event time (ms) of the phases of the removals and subtractions since the last read: ms_phase[4] = validate,
 * apply (and its undoing after a refusal), check, compact (keep flags, ids, records, the table's refill);
 * *launches = timed regions */
int mc_timing_read_voxel_remove(mc_ctx* ctx, double* ms_phase, int64_t* launches);

/* ---- surface normals of the voxel cloud (csrc/normals_core.hpp, normals.hpp) ---------------------
 * The reference's viewer runs, on every cloud without normals (read_pointcloud.py:81-84),
 *   pcd.estimate_normals(search_param=KDTreeSearchParamHybrid(radius=0.1, max_nn=30))
 * This is that estimate for the voxel points of the live build, defined so that it is a function of
 * the voxel set alone: the same bit for bit whatever order the points arrived in.  Per voxel i with
 * integer cell k_i and centroid c_i (the float64 c of the voxel filter above, those exact bits), with
 * h the build's voxel size, R = ceil(radius / h) and r2 = radius * radius; every line ONE IEEE float64
 * operation, no contraction:
 *   candidates  the occupied cells k_j with max_axis |k_j - k_i| <= R, i itself included (open3d counts
 *               the query point), walked dkx, dky, dkz ascending = ascending packed key.  The window is
 *               part of the definition: rounding of a centroid at a cell face cannot change the set.  A
 *               window cell with an index outside [-2^20, 2^20) on any axis does not exist.
 *   radius      u = c_j - c_i     d2 = (u.x*u.x + u.y*u.y) + u.z*u.z     a neighbour when d2 <= r2
 *   cap         max_nn != 0 and more than max_nn neighbours: the max_nn with the smallest (d2, packed
 *               key) are kept (the key breaks ties; a voxel's place in the output never does)
 *   moments     over the n kept neighbours in walk order:  s += u;  P += (u.x*u.x, u.x*u.y, u.x*u.z,
 *               u.y*u.y, u.y*u.z, u.z*u.z);  then m = s / double(n), E = P / double(n),
 *               C = E - (m.x*m.x, m.x*m.y, m.x*m.z, m.y*m.y, m.y*m.z, m.z*m.z) = xx, xy, xz, yy, yz, zz
 *   normal      a unit eigenvector of C for its smallest eigenvalue (a cyclic Jacobi of + - * / sqrt)
 *   sign        with a viewpoint: n . (viewpoint - c_i) >= 0; without: the component of largest
 *               magnitude is positive (ties: the lower axis)
 *   curvature   max(l0, 0) / (C.xx + C.yy + C.zz) with l0 = n^T C n; 0 when the trace is <= 0
 *   n < 3       normal (0, 0, 1), curvature 0, whatever the viewpoint (open3d's answer); C as above
 * d_normals (M, 4) float64 nx, ny, nz, curvature and d_cov (M, 6), 16-byte aligned; d_counts (M,) = n.
 * Rows are in the cloud's order (mc_voxel_emit_f64).  Any number of calls per build, with any radii.
 * MC_ERR_INVALID before any launch: radius not finite or <= 0, radius / h > 4 (voxelise coarser or
 * shrink the radius), max_nn not 0 and not in 3..64, a viewpoint that is not finite.  No successful
 * build: MC_ERR_STATE.  M = 0: MC_OK, nothing written.  Device memory, with the voxel filter's:
 * 36 B per voxel (the centroids, written by the first call after a build, and the capped list). */
int mc_voxel_normals(mc_ctx* ctx, double radius, int32_t max_nn, const double* viewpoint, double* d_normals,
                     int32_t* d_counts, double* d_cov);
/* event time (ms) of the timed phases since the last read: ms_phase[3] = centroids (once per build),
 * window (every voxel; with the counter reset), cap (the voxels with more than max_nn neighbours;
 * launched only when there are some); *launches = timed regions */
int mc_timing_read_normals(mc_ctx* ctx, double* ms_phase, int64_t* launches);

/* ---- density clustering of the voxel cloud (csrc/cluster_core.hpp, cluster.hpp) -------------------
 * The first step of the reference's point cloud processing list, noise filtering and outlier removal
 * (docs/Comprehensive Guide.md:488-491), and the segmentation behind the object files its viewer is run
 * on (read_pointcloud.py:233-257, ..._nonground_train_wagon_01.pcd to _05.pcd): DBSCAN over the voxel
 * points of the live build.  Its noise label is the radius-outlier filter, its clusters are the
 * segments; with min_points = 1 every voxel is core and the result is Euclidean cluster extraction
 * (connected components).  With h the build's voxel size, R = ceil(eps / h) and eps2 = eps * eps; every
 * line ONE IEEE float64 operation, no contraction:
 *   neighbours  of voxel i: exactly the set of the normals above without a cap, radius = eps: the occupied
 *               cells within R of k_i on every axis (cells outside the key range do not exist) with
 *               u = c_j - c_i     d2 = (u.x*u.x + u.y*u.y) + u.z*u.z     d2 <= eps2;  i itself included.
 *               The relation is symmetric.
 *   density     the number of neighbours; weighted: the sum of the neighbours' source-point counts (the
 *               d_counts of mc_voxel_emit_f64; at most N < 2^31, an int32)
 *   core        density >= min_points
 *   cluster     a connected component of the core voxels under the neighbour relation
 *   border      a voxel that is not core and has a core neighbour joins the cluster of the core neighbour
 *               with the smallest (d2, ix), ix the place in the window walk, which ascends with the
 *               packed key (a voxel's place in the output never breaks a tie)
 *   noise       every other voxel that is not core: label -1
 *   numbering   clusters are 0 .. K - 1 in ascending order of their lowest core voxel id (a voxel's id is
 *               its place in the cloud's output), so cluster 0 is the one whose core appears first.  The
 *               lowest core id is the union-find's root; a border voxel with a lower id than every core
 *               voxel of its cluster does not number it
 * The partition is a function of the voxel set, eps, min_points and weighted alone, the numbering of
 * the cloud's order alone; neither depends on the order the device's atomics arrive in (a lock-free
 * union-find whose roots are the lowest ids of their trees; no lane waits for another), so every run
 * gives the same bits.
 * d_labels (M,) int32 and d_density (M,) int32 (may be NULL), rows in the cloud's order; *n_clusters = K
 * (may be NULL).  Any number of calls per build, with any parameters.
 * MC_ERR_INVALID before any launch: eps not finite or <= 0, eps / h > 4 (voxelise coarser or shrink the
 * radius), min_points < 1, weighted not 0 or 1, ctx NULL, d_labels NULL with M > 0.  No successful build:
 * MC_ERR_STATE.  M = 0: MC_OK, K = 0, nothing written.  Device memory, with the voxel filter's: 8 B per
 * voxel beside the normals' centroids (32 B per voxel, shared with them). */
int mc_voxel_clusters(mc_ctx* ctx, double eps, int32_t min_points, int32_t weighted, int32_t* d_labels,
                      int32_t* d_density, int64_t* n_clusters);
/* per cluster of the last mc_voxel_clusters of the live build, K rows, any may be NULL: d_voxels (K,) int32
 * voxels, d_points (K,) int64 source points, d_cell_min / d_cell_max (K, 3) int32 the bounding box of the
 * cells kx, ky, kz (inclusive).  Integer atomic sums, minima and maxima: the same on every run.  Without such
 * a clustering (none yet, or a later build or release): MC_ERR_STATE.  K = 0: MC_OK, nothing written. */
int mc_voxel_cluster_stats(mc_ctx* ctx, int32_t* d_voxels, int64_t* d_points, int32_t* d_cell_min,
                           int32_t* d_cell_max);
/* event time (ms) of the timed phases since the last read: ms_phase[5] = density, union, label, number,
 * stats; *launches = timed regions (the centroids, when a clustering is the first to need them, are timed
 * with the normals') */
int mc_timing_read_clusters(mc_ctx* ctx, double* ms_phase, int64_t* launches);

/* ---- plane segmentation of the voxel cloud and selection into a batch (csrc/plane_core.hpp, plane.hpp) ----
 * The ground filter of the reference's processing chain (read_pointcloud.py:244-257: downsampled -> aligned ->
 * ground_filtered (..._nonground) -> side_filtered -> segmented) and the step that writes a segment out: RANSAC
 * plane segmentation of the live build, the counterpart of open3d's segment_plane, and a stable compaction of
 * the cloud by a mask into a one-frame batch.  Defined op for op, integer where it can be: the same bits on every
 * run.  c_v: the build's centroids by voxel id (float64).  t = distance, K = num_iterations.  ids: the candidate
 * voxel ids, ascending (d_among NULL: all M; else the voxels whose byte is non-zero), n their number.  Every
 * float64 line ONE IEEE operation, no contraction:
 *   sampler     GOLDEN = 0x9E3779B97F4A7C15;  mix(z): z = (z ^ z>>30) * 0xBF58476D1CE4E5B9,
 *               z = (z ^ z>>27) * 0x94D049BB133111EB, z ^ z>>31  (uint64, wrapping)
 *               hypothesis k, draw j = 0, 1, 2:  r_j = mix(seed + GOLDEN * (3k + j + 1))
 *               a = mulhi64(r0, n)     b = mulhi64(r1, n - 1), b++ if b >= a
 *               c = mulhi64(r2, n - 2), c++ if c >= min(a, b), then c++ if c >= max(a, b)
 *               the samples are p0, p1, p2 = c of ids[a], ids[b], ids[c]: distinct, no rejection loop, no state
 *   hypothesis  e1 = p1 - p0   e2 = p2 - p0   n = e1 x e2, each component (u*v) - (w*x)
 *               l2 = (nx*nx + ny*ny) + nz*nz     d = -((nx*p0x + ny*p0y) + nz*p0z)     tau = (t*t) * l2
 *               valid iff l2 > 0 and l2, d, tau finite; an invalid hypothesis scores 0
 *   score       candidate v is an inlier iff s*s <= tau, s = ((nx*cx + ny*cy) + nz*cz) + d; the score is the
 *               number of inliers
 *   winner      the highest score of at least 3, ties to the lowest k; none: iteration -1, an all-zero mask,
 *               the zero model, MC_OK
 *   model       refine 0:  l = sqrt(l2)   n^ = n / l   d^ = -((n^x*p0x + n^y*p0y) + n^z*p0z); the inliers are
 *               the hypothesis's own
 *   refit       refine 1: over voxel ids 0 .. M-1 the leaves u = c_v - p0 and ux*ux, ux*uy, ux*uz, uy*uy, uy*uz,
 *               uz*uz for an inlier of the winner, +0.0 otherwise; each of the nine sums is the balanced
 *               adjacent-pair tree over the leaves padded with +0.0 to the power of two >= max(M, 256) (a
 *               function of the cloud, not of workgroups or atomics).  m = s / n_in, E = P / n_in,
 *               C = E - m m^T and the unit eigenvector of C's smallest eigenvalue as the normals compute them;
 *               q = p0 + m;  d^ = -((n^x*qx + n^y*qy) + n^z*qz); the inliers are the candidates with
 *               fabs(((n^x*cx + n^y*cy) + n^z*cz) + d^) <= t
 *   sign        the whole model is negated when the component of n^ of largest magnitude is negative (the lowest
 *               axis wins a tie), as the normals' rule; in the refit before d^ is computed
 * The sampler draws voxel ids: the result is a function of the cloud in its order and of the seed, not of the
 * voxel set alone.
 * d_among (M,) uint8 or NULL; d_inliers (M,) uint8 0 / 1 or NULL; host outputs: model[4] = n^x, n^y, n^z, d^;
 * cov[6] = C (xx, xy, xz, yy, yz, zz; zeros when not refined; may be NULL); samples[3] voxel ids (-1 without a
 * winner); stats[4] = iteration, score (the RANSAC score, also after a refit), n_inliers, refined.
 * MC_ERR_INVALID before any launch: a NULL ctx, model, samples or stats, distance not finite or <= 0,
 * num_iterations outside 1 .. 2^20, refine not 0 or 1, fewer than three voxels (M = 0 among them); after the
 * mask's scan: fewer than three candidates.  No successful build: MC_ERR_STATE.  Device memory, with the voxel
 * filter's: 5 B per voxel (9 with d_among), 80 B per hypothesis, and 72 B per 256 voxels of the padded tree,
 * beside the normals' centroids. */
int mc_voxel_plane(mc_ctx* ctx, double distance, int32_t num_iterations, uint64_t seed, int32_t refine,
                   const uint8_t* d_among, uint8_t* d_inliers, double* model, double* cov, int32_t* samples,
                   int64_t* stats);
/* the hypotheses one launch of the score phase takes (its workgroup counters); more run in further launches */
int mc_voxel_plane_chunk(void);
/* The voxels of the live build whose byte of d_mask (M,) uint8 is non-zero, in the cloud's order, into the
 * one-frame batch out: each voxel's four float32 values are what mc_voxel_emit_batch writes for it, the padding
 * of the last 256-point block as there.  out->N must equal the number of set bytes (the mask's scan counts
 * them): otherwise MC_ERR_INVALID, and out is not marked written.  No successful build: MC_ERR_STATE. */
int mc_voxel_emit_selected(mc_ctx* ctx, const uint8_t* d_mask, mc_batch* out);
/* event time (ms) of the timed phases since the last read: ms_phase[6] = compact (the candidates of a call with
 * d_among), sample, score (ceil(num_iterations / mc_voxel_plane_chunk()) launches), mask, moments, select (the
 * mask's compaction and the emit of mc_voxel_emit_selected); *launches = timed regions */
int mc_timing_read_plane(mc_ctx* ctx, double* ms_phase, int64_t* launches);

/* ---- registration against the voxel cloud (csrc/register_core.hpp, register.hpp) --------------------------------
 * How well a scan sits on the map, and the small pose correction that makes it sit better: the nearest centroid of
 * the live build for points that are not its voxels, and point-to-plane ICP on it.  The source is a batch (its
 * float32 x, y, z read as float64; frame -1: all frames as one rigid body, else that frame alone) or device float64
 * rows (x, y, z first, ld >= 3); a point's index is its place in the source.  With h and the origin the build's,
 * (R, t) the pose (4 x 4 row-major, last row 0, 0, 0, 1); every line ONE IEEE float64 operation, no contraction:
 *   move      q = R p + t, each component ((R0*x + R1*y) + R2*z) + t
 *   cell      the voxel filter's k of q (a = q - o, g = a / h, k = floor(g)); a q that is not finite or whose cell is
 *             outside [-2^20, 2^20) on an axis has no nearest voxel (id -1, d2 inf) and is not an error
 *   nearest   W = ceil(max_distance / h), r2 = max_distance * max_distance; the occupied cells within W of q's cell
 *             on every axis, walked dkx, dky, dkz ascending = ascending packed key (cells outside the key range do
 *             not exist): u = c_j - q, d2 = (u.x*u.x + u.y*u.y) + u.z*u.z; a candidate when d2 <= r2; the winner is
 *             the smallest d2, ties to the cell walked first (the lower packed key).  The implementation leaves out
 *             cells whose box is farther from q than the smallest d2 it knows (they can neither win nor tie): no
 *             output differs from the plain walk's
 *   pair      the winner v, when the normal of v was estimated from three neighbours or more (the normals above with
 *             normals_radius, max_nn and no viewpoint, computed once per call); otherwise the point has no pair (the
 *             next-nearest voxel is not tried)
 *   leaves    d = q - c_v;  r = (nx*dx + ny*dy) + nz*dz;  a = q x n, each component (u*v) - (w*x);  J = (a, n);
 *             the 21 products J_i*J_j (i <= j, row-major), the 6 products J_i*r, and r*r; +0.0 each without a pair
 *   sums      each of the 28 by the balanced adjacent-pair tree of the plane refit over the source point index, the
 *             leaves padded with +0.0 to the power of two >= max(N, 256); pairs: an integer sum
 *   step      fewer than 6 pairs: status too_few_pairs.  A x = -b by Cholesky: A = L L^T row by row (i, then j <= i),
 *             acc = A_ij, acc = acc - L_ik*L_jk for k ascending, L_ii = sqrt(acc), L_ij = acc / L_jj; a diagonal acc
 *             that is not finite or not > 0: status singular.  y_i = (-b_i - sum_k<i L_ik*y_k) / L_ii for i ascending;
 *             x_i = (y_i - sum_k>i L_ki*x_k) / L_ii for i descending, k ascending.  x = (w, v)
 *   update    hx = 0.5*w.x ..;  n = sqrt(1 + ((hx*hx + hy*hy) + hz*hz));  the quaternion (1/n, hx/n, hy/n, hz/n) as a
 *             rotation dR (diagonal 1 - 2*(yy + zz) .., off-diagonal 2*(xy - wz) ..);  R <- dR R, t <- dR t + v, each
 *             entry (a0 + a1) + a2
 *   stop      after the update: converged when (w.x*w.x + w.y*w.y) + w.z*w.z <= tol_rotation^2 and the same of v
 *             <= tol_translation^2; max_iterations when the last allowed iteration did not converge.  too_few_pairs
 *             and singular return the pose before the failed step
 * mc_voxel_nearest_*: d_ids (N,) int32 the nearest voxel's id (its row in the cloud's order) or -1, d_dist2 (N,)
 * float64 d2 or inf; transform NULL: the identity.  mc_voxel_register_*: transformation[16]; history
 * (max_iterations, 8), row i = pairs, sum r*r, w, v of iteration i (a failed step: zeros), `iterations` rows written;
 * stats[4] = pairs (of the last iteration), iterations, status (0 converged, 1 max_iterations, 2 too_few_pairs,
 * 3 singular), N.  Neither call changes the build; any number of calls per build.  One synchronisation and one copy
 * of fewer than 256 x 28 partials and the pair count per iteration; the scratch is the voxel state's (4 B per
 * source point, 36 B per voxel, 224 B per 256 source points of the padded tree) and is not reallocated by an
 * iteration.  The result is the same bits on every run.
 * MC_ERR_INVALID before any launch: a NULL ctx or output, a batch of another context, a frame outside the batch, an
 * empty source (N = 0), max_distance not finite or <= 0 or max_distance / h > 4 (voxelise coarser or shrink the
 * radius), a pose whose last row is not 0, 0, 0, 1, that is not finite or with |R^T R - I| > 1e-6 in an entry,
 * max_iterations outside 1 .. 2^16, a negative or non-finite tolerance, and the normals' own refusals.  No successful
 * build: MC_ERR_STATE.  An empty cloud (M = 0): every id is -1, and a registration ends with too_few_pairs. */
typedef struct mc_register_params {
  double max_distance;
  double normals_radius;
  double tol_rotation, tol_translation;
  double init[16];          /* the starting pose, row-major */
  int32_t max_nn;           /* of the normals: 0 or 3..64 */
  int32_t max_iterations;
} mc_register_params;
int mc_voxel_nearest_batch(mc_ctx* ctx, const mc_batch* src, int32_t frame, double max_distance,
                           const double* transform, int32_t* d_ids, double* d_dist2);
int mc_voxel_nearest_f64(mc_ctx* ctx, const double* d_rows, int64_t ld, int64_t n, double max_distance,
                         const double* transform, int32_t* d_ids, double* d_dist2);
int mc_voxel_register_batch(mc_ctx* ctx, const mc_batch* src, int32_t frame, const mc_register_params* params,
                            double* transformation, double* history, int64_t* stats);
int mc_voxel_register_f64(mc_ctx* ctx, const double* d_rows, int64_t ld, int64_t n,
                          const mc_register_params* params, double* transformation, double* history,
                          int64_t* stats);
/* time (ms) of the phases since the last read: ms_phase[5] = normals (the call's window and cap launches),
 * correspond, leaves (with the first tree level), tree (the further levels; none below 65 536 source points), solve
 * (the host's last levels, Cholesky and update, by the host's clock, counted while timing is enabled);
 * *launches = timed regions */
int mc_timing_read_register(mc_ctx* ctx, double* ms_phase, int64_t* launches);

/* ---- every frame of a batch registered against the voxel cloud in one call (csrc/register.hpp k_rg_frames_*) ------
 * F independent registrations advanced together.  The contract: for every non-empty frame f, every output of frame
 * f is bit for bit what mc_voxel_register_batch(ctx, src, f, params with init = inits[f], ...) returns.  A source
 * point's index is its place within its frame, so frame f has its own tree over the power of two >= max(N_f, 256)
 * leaves, its own pair count, its own Cholesky step and its own stop; nothing couples the frames but the cloud and
 * its normals, which are computed once per call.  A frame that has ended (converged, max_iterations, too_few_pairs,
 * singular) is not touched again while the others go on: its pose, history rows, pairs and iterations are those of
 * its last evaluated iteration.
 * inits: F x 16, one row-major 4 x 4 per frame, or NULL: params->init for every frame.  transformations: F x 16.
 * history: (F, max_iterations, 8), frame f's rows as above, the rows past its iterations +0.0.  stats: (F, 4) =
 * pairs, iterations, status, N_f per frame; status 4 (empty): a frame without points, which is no error: its
 * transformation is its init and its pairs and iterations are 0.  A batch without any point is no error either.
 * Per iteration: one launch over the points of the live frames (frame f owns its tree's first level of workgroups,
 * found through a block map; correspond and leaves in one kernel), one launch per further tree level over all the
 * frames of more than 32 768 points, one launch of a workgroup per frame for the last fewer than 256 partials, the
 * step and the frame's record, then one synchronisation and one word copied: the frames still live.  Poses, stats
 * and history are copied once, at the end.  The scratch is the voxel state's (36 B per voxel, 224 B per 256 source
 * points of every frame's padded tree, 64 B per history row, 184 B per frame) and is not reallocated by an
 * iteration.  The result is the same bits on every run.
 * MC_ERR_INVALID before any launch: what mc_voxel_register_batch refuses of ctx, params and the batch (every matrix
 * of inits held to the rule of init, the message naming the frame), a NULL output, and F x max_iterations > 2^22
 * history rows (256 MB: lower max_iterations).  No successful build: MC_ERR_STATE. */
int mc_voxel_register_frames(mc_ctx* ctx, const mc_batch* src, const mc_register_params* params, const double* inits,
                             double* transformations, double* history, int64_t* stats);
/* event time (ms) of the phases since the last read: ms_phase[4] = normals (once per call), step (correspond,
 * leaves and the first tree level of every live frame), tree (the further levels), solve (the last levels, the step
 * and the records, on the device); *launches = timed regions */
int mc_timing_read_register_frames(mc_ctx* ctx, double* ms_phase, int64_t* launches);

/* ---- rays through the voxel cloud (csrc/rays_core.hpp, rays.hpp) --------------------------------------------------
 * Which voxels of the map a new scan contradicts: the ray of every source point, from the sensor position to the
 * point, walked through the grid of the live build, and per voxel the number of rays that passed through it and the
 * number that ended in it.  A voxel many beams pass and none ends in is free space the map still believes occupied (a
 * parked wagon that has left, a person who walked through, a ghost from a bad pose): mc_voxel_remove of
 * (passed >= k and ended == 0) carves it.  The build is read and never changed.  The source is as the registration's
 * (a batch: its float32 x, y, z read as float64, padding slots no points, frame -1: every frame; or device float64
 * rows, ld >= 3); the sensor positions are in the cloud's frame.  With h and o the build's voxel size and origin;
 * every float64 line ONE IEEE operation, no contraction:
 *   grid     per axis a, for the sensor position s and the point e, the voxel filter's own lines:
 *              as = s - o   gs = as / h   ks = floor(gs)        ae = e - o   ge = ae / h   ke = floor(ge)
 *            so ke is exactly the cell an insert puts the point in
 *   skipped  a ray whose s or e the filter refuses with the intensity taken as 0.0 (a coordinate or g that is not
 *            finite, a key outside [-2^20, 2^20)), or whose walk has more than max_steps steps.  It counts nowhere,
 *            its `through` is -1, and it is counted in stats[1]: not an error, as a point without a cell is none to
 *            mc_voxel_nearest_*
 *   walk     d_a = ge_a - gs_a;  dir_a = +1 when ke_a > ks_a, -1 when ke_a < ks_a, else 0;  n_a = |ke_a - ks_a|;
 *            steps = n_x + n_y + n_z: the walk has exactly that many transitions and always ends in ke.  The j-th
 *            crossing on axis a (j = 0 .. n_a - 1) has
 *              b = double(ks_a + j * dir_a + (dir_a > 0 ? 1 : 0));  u = b - gs_a;  t_a(j) = u / d_a
 *            computed from j, never accumulated; an axis with its n_a crossings done has t_a = +inf.  Each
 *            transition takes the axis of smallest current t_a, ties to the lowest axis, and moves one cell along it.
 *            No comparison sees a NaN: n_a > 0 implies d_a != 0
 *   cells    position 0 is ks, position `steps` is ke; the cells of one walk are distinct, so a ray adds at most 1 to
 *            a voxel
 *            ended   the voxel of ke, when the cloud holds one, gets +1
 *            passed  the voxels of positions 0 .. steps - 1 - guard, where the cloud holds them, get +1 each; a guard
 *                    larger than the walk leaves none.  guard is a number of cells, integer and exact: it keeps a
 *                    beam that grazes the surface it ends on from carving that surface
 * d_passed, d_ended (M,) int32 in the cloud's order (NULL allowed when M = 0); d_through (N,) int32 in the source's
 * point order: the occupied voxels the ray was counted as passing, -1 for a skipped ray (which points lie behind
 * surfaces the map believes in); stats[4] = rays, skipped, steps (the transitions of every walked ray), 0.  The counts
 * are 32-bit integer atomic adds and a call takes fewer than 2^31 rays, so they do not depend on the order the atomics
 * arrive in: the same bits on every run.  One launch and one synchronisation per call.
 * mc_voxel_rays_batch: origins is HOST memory, n_origins rows of 3: 1 (every frame) or F (one per frame; with a
 * frame given, that frame's row is used).  mc_voxel_rays_f64: d_origins is DEVICE memory, 1 or n rows of 3; the host
 * does not read them, and a row that is not finite has its ray skipped.
 * MC_ERR_INVALID before any launch: a NULL ctx, stats, source, origins or d_through, d_passed or d_ended NULL with
 * M > 0, a batch of another context, a frame outside the batch, an empty source, 2^31 points or more, ld < 3, a count
 * of origins that is neither 1 nor F (n), host origins that are not finite, guard outside 0 .. 255, max_steps outside
 * 1 .. 2^22.  No successful build: MC_ERR_STATE.  An empty cloud (M = 0) still walks: through is 0 or -1. */
int mc_voxel_rays_batch(mc_ctx* ctx, const mc_batch* src, int32_t frame, const double* origins, int64_t n_origins,
                        int32_t guard, int32_t max_steps, int32_t* d_passed, int32_t* d_ended, int32_t* d_through,
                        int64_t* stats);
int mc_voxel_rays_f64(mc_ctx* ctx, const double* d_rows, int64_t ld, int64_t n, const double* d_origins, int64_t n_origins,
                      int32_t guard, int32_t max_steps, int32_t* d_passed, int32_t* d_ended, int32_t* d_through,
                      int64_t* stats);
/* event time (ms) of the phases since the last read: ms_phase[2] = clear (passed, ended and the counters zeroed),
 * walk; *launches = timed regions */
int mc_timing_read_voxel_rays(mc_ctx* ctx, double* ms_phase, int64_t* launches);

/* ---- kept normals: the cloud's normals carried across its edits (csrc/normals_core.hpp, normals.hpp) ---------------
 * mc_voxel_register_* compute the normals of the whole cloud on every call, and a frame changes a small part of a map.
 * A voxel's row of mc_voxel_normals is a function of the occupied cells in the (2R + 1)^3 cell window of its cell and
 * of their centroids, R = ceil(radius / h), and of nothing else: not of ids, of arrival order or of atomics.  So a
 * cloud can keep its rows for one (radius, max_nn), without a viewpoint, and an edit recomputes those it can change.
 *
 *   touched voxels T of an edit
 *     mc_voxel_insert_*, mc_voxel_merge_sums   every voxel that received at least one item, new voxels included
 *     mc_voxel_subtract_*                      every voxel that lost at least one item, emptied ones included
 *     mc_voxel_remove                          the removed voxels
 *     (a voxel is touched because an item landed in it, whether or not its centroid's bits moved)
 *   dirty set D   the voxels present after the edit whose cell k has max_axis |k - k_t| <= R for the cell k_t of some
 *                 t in T: the cell window alone, without a radius test, since the centroids before and after both
 *                 matter.  The relation is symmetric, so D is found by walking the window of every touched cell; cells
 *                 outside [-2^20, 2^20) do not exist, as in mc_voxel_normals
 *   contract      after a successful edit the kept rows of D are computed again by mc_voxel_normals's definition on the
 *                 edited cloud (radius, max_nn as kept, viewpoint NULL); the rows of every other voxel are carried over
 *                 unchanged, on a removal to the voxel's new id (the survivors' order is stable).  The kept normals and
 *                 counts are then bit for bit mc_voxel_normals(radius, max_nn, NULL) of the edited cloud, and the rows
 *                 the edit recomputed number exactly |D|, which mc_voxel_kept_info reports
 *   refusals      a refused edit (a bad item, a missing voxel, a bad remainder, 2^31 points) leaves the kept rows bit
 *                 for bit as they were and recomputes 0 rows, as does a call without items and a mc_voxel_remove whose
 *                 mask removes nothing.  An edit that fails after the cloud stopped being live leaves none kept either
 *
 * While normals are kept the centroids stay current too: an edit rewrites those of its touched voxels (a removal all
 * of them, being a pass over the cloud anyway), and no analysis after it writes them again.  An insert or a
 * subtraction that empties no voxel still makes no pass over the cloud or the table; it synchronises twice more than
 * without kept normals: for the dirty count, and (max_nn != 0) for the number of dirty voxels the cap applies to.
 * Device memory: 48 bytes per voxel (32 + 4 of rows and counts, two 4-byte stamps, 4 of the dirty list).
 *
 * mc_voxel_keep_normals computes all rows now (one full pass, timed as mc_voxel_normals's phases) and keeps them;
 * called again it replaces them.  It refuses what mc_voxel_normals refuses of radius and max_nn.  A cloud of no
 * voxels may keep normals: a later insert refreshes every new voxel.  A new mc_voxel_build_* on the context,
 * mc_voxel_release and mc_voxel_drop_normals end them, and each gives their memory back.  mc_voxel_register_* and
 * mc_voxel_register_frames read the kept rows, and launch no normals kernel, when the call's normals_radius and max_nn
 * equal the kept ones (the radius compared as bits); otherwise they run as without, and the kept rows stay as they are.
 * mc_voxel_normals is always the full, fresh computation. */
int mc_voxel_keep_normals(mc_ctx* ctx, double radius, int32_t max_nn);
/* copies of the kept rows (M, 4) = nx, ny, nz, curvature and counts (M,) into device memory (either may be NULL);
 * MC_ERR_STATE when none are kept */
int mc_voxel_kept_normals(mc_ctx* ctx, double* d_normals, int32_t* d_counts);
/* the kept parameters, and counters[3] since the build: full passes run, rows recomputed by the last edit (|D|), rows
 * recomputed by all edits; any may be NULL; MC_ERR_STATE when none are kept */
int mc_voxel_kept_info(mc_ctx* ctx, double* radius, int32_t* max_nn, int64_t* counters);
int mc_voxel_drop_normals(mc_ctx* ctx);
/* event time (ms) of the refresh phases since the last read: ms_phase[4] = mark (claim, centroid, window marking),
 * window, cap, carry (a removal's compaction of the kept rows); *launches = timed regions */
int mc_timing_read_kept_normals(mc_ctx* ctx, double* ms_phase, int64_t* launches);

/* Synthetic Mid-70 frames generated on the device (counter-hash RNG, bit-identical to
 * oracle/synth.py): frame f uses seed  seed + frame_id_base + f. */
int mc_batch_synth(mc_batch* b, uint64_t seed, int64_t frame_id_base);
/* float64 sums of x, y, z, intensity, t_ns over the valid points (deterministic order) */
int mc_batch_checksum(mc_batch* b, double* sums5);

/* ---- the hot path --------------------------------------------------------- */
/* out must have the same frame counts as in (it may be the same batch: in-place).
 * Per-point modes: when the input's time column was written since its spans were last computed, the
 * call first queues the span pass and waits for one word of it (is every frame evenly timed?
 * mc_batch_time_rule): one synchronisation per write of the time column, none on later calls.
 *
 * The intensity column.  Every deskew passes it through unchanged.  A per-point launch (mc_deskew,
 * mc_deskew_steps, mc_deskew_relative, mc_tune_order) into a batch without MC_BATCH_WITH_PCD_LEN and
 * without a pcd_len target neither reads nor writes the column when the output already holds it:
 *   - out == in (in place), from the first call;
 *   - out received a deskew of `in` before (any mode) and neither batch's x|y|z|intensity columns have
 *     been written since by anything else: the same scans deskewed again after mc_set_trajectory, in
 *     another mode, with another t_ref, or the later steps of mc_deskew_steps.
 * Such a launch moves 24 bytes per point instead of 32 (28 instead of 36 when the time column is read);
 * the output is the same to the byte, padding slots included.  The first deskew of a fresh (in, out)
 * pair moves what it always did.  Every write of either batch's point columns (uploads, synth, the
 * stagers, affine, decoders, emits, gathers, a deskew of another input into out) ends the state; a new
 * batch never matches an old one.  Frame mode always moves the column.
 * mc_batch_holds_intensity_of(out, in): 1 when out holds in's intensity column right now, else 0 (< 0:
 * a NULL argument); a pure query of host state, nothing is queued or waited for.
 * mc_set_keep_intensity(ctx, 0) makes every later launch of the context take the full kernels (1: back
 * to the default); the environment variable MCDESKEW_KEEP_INTENSITY=0 creates contexts with it off. */
int mc_deskew(mc_ctx* ctx, const mc_batch* in, mc_batch* out, int mode, int pose_select);
int mc_batch_holds_intensity_of(const mc_batch* out, const mc_batch* in);
int mc_set_keep_intensity(mc_ctx* ctx, int enable);

/* The SLERP deskew into the SENSOR frame at a reference time per frame (build-added, as SURVEY §8a
 * row a11 is): with (R_ref, pos_ref) = the SLERP / LERP pose of the trajectory at t_ref[f] (seconds,
 * the pose table's time base, clamped to the table exactly as a point's time is),
 *   p' = R_ref^T ( R(q(t)) p + pos(t) - pos_ref ),   t = frame_time[f] + t_ns * 1e-9,
 * x, y, z formed in float64 and rounded once to float32 on the store; intensity and t_ns pass through
 * as in mc_deskew.  The inverse reference pose is folded into the frame's pose records once per frame
 * and segment (in float64, where pos - pos_ref cancels), so the per-point work and the bytes moved are
 * those of mc_deskew(MC_MODE_POSE_SLERP), and a float32 batch stays exact for GPS / UTM-scale
 * trajectories.  A point whose time equals t_ref[f] comes back as itself; p_global = R_ref p' + pos_ref
 * with the pose of mc_pose_at(t_ref[f]).  t_ref[n_frames] is a host array, copied and not retained;
 * NULL: each frame's own time (mc_batch_set_frame_times), i.e. frame start.  Preconditions and error
 * codes of mc_deskew(MC_MODE_POSE_SLERP); a non-finite t_ref -> MC_ERR_INVALID.  out may be in.
 * Asynchronous on the context stream like mc_deskew, after a first call that sizes the batch's
 * relative table (one synchronisation; again when the trajectory, the frame times, t_ns or t_ref
 * change).  No mc_deskew_steps / mc_deskew_pcd / mc_tune_order variants and no IMU-mode variant. */
int mc_deskew_relative(mc_ctx* ctx, const mc_batch* in, mc_batch* out, const double* t_ref);

/* The pose the library interpolates at n arbitrary finite times t (seconds): R (n, 3, 3) row-major and
 * pos (n, 3), quaternion SLERP + position LERP of the uploaded trajectory, clamped to the table — the
 * device function that builds mc_deskew_relative's reference poses (build-added, like a11).
 * A non-finite time -> MC_ERR_INVALID; no trajectory -> MC_ERR_STATE.  Synchronous. */
int mc_pose_at(mc_ctx* ctx, int64_t n, const double* t, double* R, double* pos);

/* Per-frame [min, max] of t_ns over the frame's valid points, as the library keeps them for the
 * per-point modes (computed here if stale): t_min[n_frames], t_max[n_frames]; an empty frame has
 * min > max.  A frame-end reference is frame_time[f] + t_max[f] * 1e-9.  A batch without
 * MC_BATCH_WITH_TIME -> MC_ERR_STATE.  Synchronous. */
int mc_batch_time_spans(mc_batch* b, int32_t* t_min, int32_t* t_max);

/* The evenly-timed rule (csrc/time_rule.hpp).  Frame f with n valid points is evenly timed when
 * t_ns[i] == t0 + i * dt for every valid i, with t0 = t_ns[0] and dt = t_ns[1] - t_ns[0] (0 for
 * n < 2), all in int32 wrap-around arithmetic; an empty frame is evenly timed.  The pass that keeps
 * the time spans tests every valid point, so the rule is current exactly when the spans are (every
 * write of the time column makes both stale).  When every frame of an input batch is evenly timed,
 * the per-point modes (mc_deskew, mc_deskew_steps, mc_deskew_pcd, mc_deskew_relative, mc_tune_order)
 * launch kernels that form each point's time from (t0, dt) and its index and do not read the column:
 * 32 instead of 36 bytes per point, the outputs the same to the bit.  A batch with one frame off its
 * ramp keeps the loading kernels.
 * mc_batch_time_rule: even[n_frames] (1 / 0), t0[n_frames], dt[n_frames], computed here if stale.  A
 * batch without MC_BATCH_WITH_TIME -> MC_ERR_STATE.  Synchronous.
 * mc_set_time_rule(ctx, 0) makes every later launch of the context take the loading kernels (1: back
 * to the default); the environment variable MCDESKEW_TIME_RULE=0 creates contexts with it off. */
int mc_batch_time_rule(mc_batch* b, int8_t* even, int32_t* t0, int32_t* dt);
int mc_set_time_rule(mc_ctx* ctx, int enable);

/* Measure, on this device, which sub-tile order streams the mode's deskew kernel faster for batches
 * shaped like `in` (dealt over the 8 XCDs vs XCD-contiguous: the faster one differs between MI355X
 * boxes by up to 7 %) and use it for every later launch of that mode on batches of the same padded
 * size.  Runs the kernel `launches` times per order and round (in -> out, out != in; the results do
 * not depend on the order), alternating the orders over `rounds`.  us_out[2] (may be NULL) receives
 * the median microseconds per launch of {dealt, XCD-contiguous}; *chosen (may be NULL) the order
 * kept (0 / 1; -1 for an empty batch): the mode's default order unless the other one is at least
 * 1 % faster.  Synchronous. */
int mc_tune_order(mc_ctx* ctx, const mc_batch* in, mc_batch* out, int mode, int pose_select, int32_t launches,
                  int32_t rounds, double* us_out, int32_t* chosen);
/* n_steps consecutive mc_deskew calls (same arguments), LMC:802-832 n times over one batch, as
 * n + 1 launches: step 0's pose prep, then n deskew launches of which the first n - 1 also run the
 * next step's prep in their first workgroups (every step runs its own prep, one launch ahead, into
 * the other table half).  sample_every > 0 puts timing events around the kernels of every
 * sample_every-th step (read by mc_timing_read).  Asynchronous. */
int mc_deskew_steps(mc_ctx* ctx, const mc_batch* in, mc_batch* out, int mode, int pose_select, int32_t n_steps,
                    int32_t sample_every);

/* One call of transform_pointcloud (LMC:772-776) on host arrays: points (n, ld>=4) float64 rows,
 * rpy / translation (3,) float64 -> out (n, 4) float64 = [R p + t, intensity], bit-identical to the
 * reference's float64 result (R as scipy's from_euler('xyz').as_matrix(), numpy's matmul
 * accumulation).  Below 32768 rows the kernel reads and writes pinned, device-mapped host memory (no
 * DMA round trips); a lone ~1.6k-row call still costs ~14 us against numpy's ~9.5 (INTEGRATION.md:
 * batch the frames).  ld < 4 -> MC_ERR_INDEX. */
int mc_transform_pointcloud_f64(mc_ctx* ctx, const double* points, int64_t n, int64_t ld, const double* rpy,
                                const double* translation, double* out);

/* Host only (no device): R (n, 3, 3) row-major of Rotation.from_euler('xyz', rpy[i]).as_matrix() for
 * each rpy (n, 3) — scipy 1.15's arithmetic repeated operation for operation, equal bit for bit.  The
 * per-frame rotation basis of every float64 path (LMC:726, 774). */
int mc_rotation_from_euler_xyz(int64_t n, const double* rpy, double* R);

/* The per-point modes on the reference's own float64 data (no float32 staging): MotionCompensator.
 * compensate_point_cloud / apply_motion_compensation (CSIM:1435-1480, 2086-2105) for MC_MODE_IMU,
 * the per-point SLERP deskew for MC_MODE_POSE_SLERP.  points (N, ld >= 3) float64 rows, frames back
 * to back (counts[f] rows each); t_ns (N,) int64 = each point's time minus its frame's start (any
 * int64: no int32 limit here); frame_times[F] (s, SLERP: t = frame_times[f] + t_ns * 1e-9) or
 * frame_start_ns[F] (IMU: the point's timestamp = frame_start_ns[f] + t_ns, CSIM:1447, 1454).  out
 * (N, 4) float64 = x', y', z' computed in float64 end to end, column 3 = points[:, 3] (0 when ld == 3).
 * Pose / IMU tables from mc_set_trajectory / mc_set_imu.  ld < 3 -> MC_ERR_INDEX.  Synchronous. */
int mc_deskew_points_f64(mc_ctx* ctx, int mode, int32_t n_frames, const int64_t* counts, const double* points,
                         int64_t ld, const int64_t* t_ns, const double* frame_times, const int64_t* frame_start_ns,
                         double* out);

/* mc_deskew_relative's contract on float64 rows (build-added, like a11): the arguments of
 * mc_deskew_points_f64(MC_MODE_POSE_SLERP) plus t_ref[n_frames] (NULL: frame_times).  Computed by
 * the direct formula, not the folded records: per point the global float64 value, minus pos_ref, then
 * R_ref^T — an independent check of the batch path.  A non-finite t_ref -> MC_ERR_INVALID.
 * Synchronous. */
int mc_deskew_points_relative_f64(mc_ctx* ctx, int32_t n_frames, const int64_t* counts, const double* points,
                                  int64_t ld, const int64_t* t_ns, const double* frame_times, const double* t_ref,
                                  double* out);

/* The frame loop (LMC:802-832) on host arrays: frames[f] (counts[f], lds[f] >= 4) float64 rows
 * -> outs[f] (counts[f], 4) float64, pose per frame from the uploaded trajectory (pose_select as
 * mc_deskew's frame mode; frame_times for MC_POSE_SEARCHSORTED), float64 math, one launch over
 * all frames on pinned, device-mapped host memory (host copies on 16 threads above 8 MB). */
int mc_align_frames_host_f64(mc_ctx* ctx, int32_t n_frames, const double* const* frames, const int64_t* counts,
                             const int64_t* lds, const double* frame_times, int pose_select, double* const* outs);

/* CoordinateTransformer.transform_points (CSIM:153-233) / _transform_coordinates (CSIM:2107-2163):
 * p' = A p + b with one 3x4 [A | b] matrix (row-major float64, 12 values) for all frames
 * (n_mats == 1) or one per frame (n_mats == n_frames).  w_column != 0: the intensity column is the
 * homogeneous w of (N,4) input (p' = A p + b w, CSIM:226-229).  The 4th column passes through.
 * Synchronous; timed with the deskew kernels (mc_timing_read main). */
int mc_transform_affine(mc_ctx* ctx, const mc_batch* in, mc_batch* out, int32_t n_mats, const double* mats,
                        int w_column);
/* The same on the caller's float64 rows, bit-identical to the reference (numpy's accumulation of
 * (T @ points_h.T).T, CSIM:230): rows (N, ld) with ld 3 (w = 1, CSIM:223-225) or 4 (the 4th column is
 * w, CSIM:227), frames back to back (counts[f] rows); mats = 3x4 [A | b] row-major, 1 or n_frames of
 * them; out (N, 3) float64 (CSIM:233).  A frame is one transform_points call: numpy sums a one-row
 * call (a matrix-vector product) in another order than a larger one, and both are repeated.  per_row
 * = MC_AFFINE_PER_ROW treats every row as its own call — _transform_coordinates' per-point loop
 * (CSIM:2117-2141); MC_AFFINE_TRANSLATE adds b to each row's x, y, z and ignores A — that loop's UTM
 * branch, point + [utm_x, utm_y, 0] (CSIM:2132), one rounding per coordinate (no products, so a
 * non-finite coordinate does not spread to the others).  Synchronous. */
#define MC_AFFINE_PER_FRAME 0
#define MC_AFFINE_PER_ROW 1
#define MC_AFFINE_TRANSLATE 2
int mc_affine_rows_f64(mc_ctx* ctx, int32_t n_frames, const int64_t* counts, const double* rows, int64_t ld,
                       int32_t n_mats, const double* mats, int per_row, double* out);

/* HIP-event timing of the hot kernels (main deskew kernel and the pose-prep kernel) */
int mc_timing_enable(mc_ctx* ctx, int enable);
int mc_timing_read(mc_ctx* ctx, double* main_ms_total, int64_t* main_launches,
                   double* prep_ms_total, int64_t* prep_launches);
/* the main kernels' event times one by one (ms, in launch order; up to cap of them, *n = how many
 * were pending); those events are released (the prep / layout / codec ones stay for mc_timing_read) */
int mc_timing_read_each(mc_ctx* ctx, double* main_ms, int64_t cap, int64_t* n);
/* the same timed deskew launches' own execution spans (us, launch order; up to cap, *n = how many):
 * first workgroup start to last workgroup end on the wall clock, without the dispatch gap a start
 * event ahead of a launch includes; released */
int mc_timing_read_spans(mc_ctx* ctx, double* us, int64_t cap, int64_t* n);
/* kernel tuning knobs: 0 keeps the default */
int mc_set_launch(mc_ctx* ctx, int32_t max_grid);

/* ---- multi-GPU merged-cloud gather over RCCL/xGMI (LMC:887-889 vstack) ---- */
int mc_comm_unique_id(char id_out[128]);
int mc_comm_init(mc_ctx* ctx, int nranks, int rank, const char id[128], mc_comm** out);
int mc_comm_destroy(mc_comm* comm);
/* ragged gather of every rank's batch columns (x,y,z,intensity; blocked layout) into `merged`
 * on `root`, in rank order (== np.vstack of the frame-ordered shards).  `merged` is ignored on
 * non-root ranks and on root must have been created with the concatenated frame counts. */
int mc_comm_gather_batch(mc_comm* comm, const mc_batch* local, int root, mc_batch* merged);
int mc_comm_allreduce_max_f64(mc_comm* comm, double* values, int64_t n);
/* Host only (no device work): the plan mc_comm_gather_batch follows for n ranks whose shards hold
 * padded[q] points of columns[q] (4 or 5) values per block into a merged batch of merged_padded
 * points and merged_columns columns: offset_out[q] = the shard's first padded point in the merged
 * batch (rank order == np.vstack order, LMC:887-889), stage_offset_out[q] = its value offset in the
 * root's staging area (-1: received in place), *stage_values_out = staging size.  Invalid plans
 * (sizes that do not add up, a shard with fewer columns than the merged batch) -> MC_ERR_INVALID. */
int mc_gather_plan(int32_t nranks, int32_t root, const int64_t* padded, const int64_t* columns, int64_t merged_padded,
                   int32_t merged_columns, int64_t* offset_out, int64_t* stage_offset_out, int64_t* stage_values_out);
/* The same merge inside one process: n shard batches of one context into `merged` (created with the
 * concatenated frame counts), shard `root` playing the root's own batch and device copies standing
 * in for the RCCL receives — the plan, staging and re-pitch of mc_comm_gather_batch.  Synchronous. */
int mc_gather_batches(mc_ctx* ctx, int32_t n, const mc_batch* const* shards, int32_t root, mc_batch* merged);

#ifdef __cplusplus
}
#endif
#endif /* MCDESKEW_H_ */
