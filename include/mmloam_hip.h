/*
 * mmloam_hip.h -- C-ABI of libmmloam_hip.so: the MI355X (gfx950) implementation of the mm-loam
 * scan-registration hot path.
 *
 * The reference (TIERS/multi-modal-loam) has no plugin / FFI surface: the path sits behind two C++
 * classes.  This header defines the boundary directly beneath them; every entry point cites the
 * reference member it replaces (paths relative to /root/reference/mm-loam/).  The C++ adapter
 * (multi-modal-loam_amd/host/mmloam_adapter.hpp) re-creates the reference's method signatures on
 * top of these calls; INTEGRATION.md shows the binding a maintainer adds inside the catkin package.
 *
 * Conventions
 *   - plain C types only; the caller owns every buffer it passes, the library owns the opaque
 *     mml_ctx (device allocations, maps, one HIP stream).  One ctx per caller thread / per GPU.
 *   - every function returns 0 on success, < 0 on error (mml_status); mml_last_error(ctx) gives
 *     a message.  No exceptions cross the boundary.  There is NO CPU fallback: without a HIP
 *     device mml_create fails with MML_ERR_NO_DEVICE.
 *   - work is batched: a ctx holds `max_scans` scan slots; the reference's one-scan-at-a-time
 *     use is slot 0, count 1.  Calls are stream-ordered on the ctx stream; functions that copy
 *     results to host memory synchronise that stream before returning.
 *   - matrices are row-major doubles; quaternions are (x, y, z, w).
 */
#ifndef MMLOAM_HIP_H
#define MMLOAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MML_ABI_VERSION 1

typedef enum {
    MML_OK = 0,
    MML_ERR_INVALID = -1,   /* bad argument (null, out of range, wrong state) */
    MML_ERR_NO_DEVICE = -2, /* no HIP device / device index out of range */
    MML_ERR_HIP = -3,       /* a HIP runtime call failed */
    MML_ERR_CAPACITY = -4,  /* input exceeds a capacity fixed in mml_config */
    MML_ERR_STATE = -5      /* call order violated (e.g. estimate before a map was set) */
} mml_status;

typedef struct mml_ctx mml_ctx;

/* livox_ros_driver/CustomPoint as laid out by roscpp (20 bytes): pass msg->points.data(). */
typedef struct {
    uint32_t offset_time;
    float x, y, z;
    uint8_t reflectivity, tag, line, _pad;
} mml_livox_point;

typedef struct {
    int max_scans;          /* scan slots (batch capacity) */
    int max_velo_points;    /* per slot */
    int max_livox_points;   /* per slot */
    int n_rings;            /* VELO_N_SCANS, unionFeatureExtract.cpp:192 (16) */
    float pitch0_deg;       /* -15: ring = int((pitch - pitch0) / pitch_step + 0.5), :1162 */
    float pitch_step_deg;   /* 2 */
    int n_livox_lines;      /* 6, unionFeatureExtract.cpp:906,959 */
    float near_th, far_th;  /* near/far_points_threshold, mm_lio_full.launch:28-29 (2.0 / 50.0) */
    float leaf_corner;      /* filter_parameter_corner, launch:43 (0.4), Estimator.cpp:78 */
    float leaf_surf;        /* filter_parameter_surf,   launch:44 (0.2), Estimator.cpp:79 */
    float cell_corner;      /* kNN grid cell edge for the corner map, metres (<=0: 5 * leaf) */
    float cell_surf;        /* kNN grid cell edge for the surf map (<=0: 5 * leaf) */
    int max_features;       /* per slot per kind after down-sampling (<=0: 8192) */
    int max_map_points;     /* per map (<=0: 1<<21) */
} mml_config;

/* Fills the reference's shipped parameters (launch/mm_lio_full.launch) for `max_scans` slots. */
void mml_config_default(mml_config* cfg, int max_scans);

int mml_abi_version(void);
int mml_create(const mml_config* cfg, int device, mml_ctx** out);
void mml_destroy(mml_ctx* ctx);
const char* mml_last_error(const mml_ctx* ctx);
/* The configuration the context was created with, defaults resolved (cell sizes, max_features, max_map_points). */
int mml_config_get(const mml_ctx* ctx, mml_config* out);
int mml_synchronize(mml_ctx* ctx);

/* ---- input ------------------------------------------------------------------------------------
 * Host -> device copy of one union_cloud message (union-cloud/msg/union_cloud.msg: velo_time_aligned
 * as packed x,y,z,intensity floats, livox_time_aligned.points) into a slot.  Either part may be
 * empty (n = 0).  Asynchronous on the ctx stream (the host buffers must stay valid until the next
 * synchronising call). */
int mml_scan_upload(mml_ctx* ctx, int slot, const float* velo_xyzi, int n_velo,
                    const mml_livox_point* livox, int n_livox);

/* Many scans per copy, for a feeder that stages a batch in two host arrays laid out like the slots themselves: scan i of
 * the call (slot first_slot + i) has its n_velo[i] x (x, y, z, intensity) floats at velo_base + i * max_velo_points * 4
 * and its n_livox[i] CustomPoint records at livox_base + i * max_livox_points (max_* as given to mml_create, which must be
 * multiples of 64 for this entry point).  Two host-to-device copies for the whole batch instead of two per scan: at
 * 0.46 MB per copy the per-scan entry point reaches ~11 GB/s, this one the PCIe rate.  Asynchronous like mml_scan_upload,
 * and on a copy stream of its own: the copies start after everything enqueued before the call, the next entry point that
 * touches one of these slots waits for them, and work enqueued on OTHER slots runs concurrently with them -- a feeder
 * that alternates two slot ranges (upload range B, then mml_step on range A, and vice versa) hides the PCIe time behind
 * the kernels. */
int mml_scan_upload_batch(mml_ctx* ctx, int first_slot, int count, const float* velo_base, const int* n_velo,
                          const mml_livox_point* livox_base, const int* n_livox);

/* Same, with the Velodyne part taken straight from a sensor_msgs/PointCloud2 payload (SURVEY section 8(f) rank 3;
 * replaces pcl::fromROSMsg at unionFeatureExtract.cpp:1119-1121): data = msg.data.data(), n_points = width * height,
 * point_step and the byte offsets of the float32 fields x, y, z, intensity as listed in msg.fields
 * (off_intensity < 0: no such field, 0 is used).  The records are decoded on the device. */
int mml_scan_upload_pointcloud2(mml_ctx* ctx, int slot, const uint8_t* data, int n_points, int point_step, int off_x,
                                int off_y, int off_z, int off_intensity, const mml_livox_point* livox, int n_livox);
/* Same again, with the Livox part in wire form as well: `livox_wire` is the serialised `points` array of a
 * livox_ros_driver/CustomMsg (the bytes after its 4-byte length prefix), 19 bytes per CustomPoint, little endian:
 * uint32 offset_time, float32 x, y, z, uint8 reflectivity, tag, line -- the fields getHoriFeatureExtract reads at
 * unionFeatureExtract.cpp:985-997.  For callers that hold the raw message (a bag reader, a non-roscpp transport); a
 * roscpp callback already holds the 20-byte structs mml_scan_upload takes.  Decoded on the device. */
int mml_scan_upload_wire(mml_ctx* ctx, int slot, const uint8_t* data, int n_points, int point_step, int off_x, int off_y,
                         int off_z, int off_intensity, const uint8_t* livox_wire, int n_livox);
/* The fused labelled cloud of a slot as the payload pcl::toROSMsg(pcl::PointCloud<PointXYZINormal>) produces for
 * velo_combine / livox_combine (unionFeatureExtract.cpp:918, :1287-1293): 48-byte records, float32 fields x 0, y 4,
 * z 8, normal_x 16 (in-sweep time), normal_y 20 (ring / line), normal_z 24 (label 0/1/2), intensity 32,
 * curvature 36; packed on the device.  out may be NULL to query *n_points only. */
int mml_scan_download_pointxyzinormal(mml_ctx* ctx, int slot, uint8_t* out, int capacity_points, int* n_points);

/* The way INTO a slot for a labelled cloud that was extracted elsewhere -- the PoseEstimation process receives
 * velo_combine / livox_combine over /union_feature_cloud (unionPoseEstimation.cpp:679-688: pcl::fromROSMsg into
 * laserCloudFullVeloRes / laserCloudFullHoriRes, merged at :746-757) and hands the cloud to RemoveLidarDistortion(cloud,
 * dR, dt) (:862) and, inside a LidarFrame (Estimator.h:33-56), to EstimateLidarPose (:872).  Inverse of
 * mml_scan_download_pointxyzinormal: n_points 48-byte PointXYZINormal records (msg.data.data(), velo_combine followed
 * by livox_combine; the first n_velo are the Velodyne part), decoded on the device: normal_x -> in-sweep time,
 * normal_y -> ring / line, normal_z -> label by abs(normal_z - k) < 1e-5 (Estimator.cpp:995-1003; anything else 0),
 * intensity kept.  Afterwards the slot is in the state mml_extract leaves (mml_scan_info_get, mml_undistort,
 * mml_downsample, mml_estimate work on it); livox_*_num count the kept points only.  Synchronous.
 * (`count` whole union_cloud messages in one call, the merge decision of :741-773 included: mml_pose_ingest_batch below.) */
int mml_cloud_upload(mml_ctx* ctx, int slot, const uint8_t* pointxyzinormal, int n_points, int n_velo);

/* The registered cloud: the fused cloud of `count` slots moved into the world frame, the payload of /velo_full_cloud_mapped
 * (unionPoseEstimation.cpp:896-911).  Slot first_slot + i goes through pointAssociateToMap (:199-213) with pose i of T_wl
 * (count row-major 4x4 matrices: transformTobeMapped of :876-880); the upper three rows are applied as given, orthonormal
 * or not.  n_points[i] is the slot's fused point count (what mml_scan_info_get returns), its records start at record
 * n_points[0] + ... + n_points[i-1] of `out`, in the fused order of mml_scan_download_pointxyzinormal (Velodyne part,
 * then Livox); a slot without points contributes none.  out == NULL: only n_points is filled (the sizing call).
 * Each record is the 48-byte PointXYZINormal the reference's loop pushes back -- a default-constructed point that receives
 * five fields, which is NOT the record of mml_scan_download_pointxyzinormal (that one carries the in-sweep time in normal_x
 * and the ring / line in normal_y; both are 0 here, as in the reference's message):
 *   x, y, z (floats 0-2): in double, (R[r][0] x + R[r][1] y) + R[r][2] z, then + t[r] -- Eigen's order for
 *       topLeftCorner(3,3) * pin + topRightCorner(3,1), no fused multiply-add -- rounded once to float;
 *   float 3 = 1; normal_x = normal_y = 0 (floats 4, 5); normal_z (float 6) = the label 0 / 1 / 2; float 7 = 0;
 *   intensity (float 8) carried over; curvature and padding (floats 9-11) = 0.
 * The slots are read as they stand (undistorted or not: the reference passes the undistorted cloud, the order of the calls
 * is the caller's) and nothing in them is modified; slots filled by mml_extract and by mml_cloud_upload both work.
 * One kernel launch for the whole call and TWO host synchronisations whatever `count` is (the counts of all slots in one
 * copy; the records in one copy), one for the sizing call.  MML_ERR_CAPACITY, before any record is written, when
 * capacity_points is below the total; MML_ERR_INVALID for a slot range outside the context, count < 1 (or above 65535),
 * NULL T_wl or NULL n_points; MML_ERR_HIP, before any launch, when the device staging cannot be grown to the total. */
int mml_cloud_download_registered_batch(mml_ctx* ctx, int first_slot, int count, const double* T_wl /* count x 16 */,
                                        uint8_t* out, long capacity_points, int* n_points /* count */);
/* One slot: the count = 1 case of the batch call (the same code path). */
int mml_cloud_download_registered(mml_ctx* ctx, int slot, const double* T_wl /* 16 */, uint8_t* out, int capacity_points,
                                  int* n_points);

/* The world map: the registered clouds above voxel-merged ON the device, one map per sequence, n_maps (1 .. 1024 =
 * MML_MAP_BANKS_MAX) maps per context numbered like the banks -- what a replay keeps of /velo_full_cloud_mapped where the
 * reference leaves the accumulation to a recorder.  One hash table of voxels holds all maps; the work of an add does not depend
 * on how much the maps hold.  The arithmetic is defined once, in csrc/world_map_key.h (host and device):
 *   world point   the slot's fused point through the function mml_cloud_download_registered_batch uses (double, Eigen's order,
 *                 no fused multiply-add, rounded once to float); intensity carried over;
 *   voxel index   per axis i = (int)floor((double)(x * inv)), inv = 1.0f / leaf and the product in float.  A point is SKIPPED
 *                 and counted when its label is not in label_mask (n_masked), else when a coordinate or the intensity is not
 *                 finite (n_nonfinite), else when an index is outside [-2^17, 2^17) (n_out_of_range; the one voxel
 *                 (2^17-1, 2^17-1, 2^17-1) of map 1023, whose key would be the table's empty marker, counts as outside too);
 *   voxel         float sums of x, y, z, intensity and a count.  A voxel's points are added one after the other in float,
 *                 starting from the stored sum, in call order, then slot order inside the call, then fused point order inside
 *                 the slot; the centroid is sum / (float)count per field.
 * mml_world_map_create: once per context (MML_ERR_STATE if present); capacity_voxels (1 .. 2^29) is the total over all maps,
 * 28 bytes per table position at 2 .. 4 positions per voxel.  _destroy frees it (mml_destroy does too); _reset empties one map
 * (the others keep every bit of theirs) or, map = -1, all.  _size: the voxels of one map, or of all (map = -1).
 * mml_world_map_add: slot first_slot + i into map map_of_slot[i] (-1: the slot is skipped) at pose i of T_wl (row-major 4x4,
 * the upper three rows applied as given).  label_mask bit l: the points labelled l take part (0 none, 1 corner, 2 surf; 7 = all).
 * The slots are read as they stand and never modified; slots filled by mml_extract and by mml_cloud_upload both work.  `info`
 * (may be NULL) receives the call's counts: n_points = n_kept + n_nonfinite + n_out_of_range + n_masked over the slots that
 * take part, the voxels the call created and the total of all maps after it.  One chain of launches and ONE host synchronisation
 * whatever `count` is.  BATCHING GUARANTEE: one call over `count` slots leaves exactly the bytes that `count` calls of one slot
 * each, in slot order, leave -- every map's download and the sums of the info counts.  Refused before anything is written to
 * the table: MML_ERR_STATE without a map; MML_ERR_INVALID for a slot range outside the context, count outside 1 .. 65535, a map
 * number outside [-1, n_maps), NULL map_of_slot / T_wl, label_mask & 7 == 0; MML_ERR_HIP when the scratch (52 bytes per point
 * of count x the context's points per slot, grow-only) cannot grow; MML_ERR_CAPACITY, naming the figures, when the voxels held
 * plus the call's new ones exceed capacity_voxels -- the table is then bit for bit what it was and a smaller call still works.
 * mml_world_map_download: the voxels of one map in ascending key order (z index, then y, then x) as centroids x, y, z,
 * intensity (4 floats each) and, out_count != NULL, their point counts.  out_xyzi == NULL: only *n_voxels (the sizing call);
 * MML_ERR_CAPACITY when `capacity` (voxels) is below it.  Which table position a voxel occupies may differ from run to run;
 * nothing a call returns depends on it. */
typedef struct {
    long n_points, n_kept, n_nonfinite, n_out_of_range, n_masked, n_new_voxels, n_voxels_total;
} mml_world_map_info;
int mml_world_map_create(mml_ctx* ctx, int n_maps /* 1..1024 */, float leaf, long capacity_voxels);
int mml_world_map_destroy(mml_ctx* ctx);
int mml_world_map_reset(mml_ctx* ctx, int map /* -1: all */);
int mml_world_map_add(mml_ctx* ctx, int first_slot, int count, const int* map_of_slot /* count; -1 skips the slot */,
                      const double* T_wl /* count x 16 */, unsigned label_mask /* bit l: label l takes part; 7 = all */,
                      mml_world_map_info* info /* may be NULL */);
int mml_world_map_size(mml_ctx* ctx, int map /* -1: all */, long* n_voxels);
int mml_world_map_download(mml_ctx* ctx, int map, float* out_xyzi, int* out_count /* may be NULL */, long capacity, long* n_voxels);

/* Surfel maps: per-voxel scatter, normals and planarity on the device, opt-in per context.  mml_world_map_create_opts with
 * flags = MML_WM_SURFELS creates a world map whose table holds 12 floats of moments per position beside the sum and the count,
 * 76 bytes per position instead of 28; flags = 0 IS mml_world_map_create (the same code path, the same 28 bytes, every download
 * byte-identical); unknown flag bits: MML_ERR_INVALID.  Every other call works on both kinds; an add into a surfel map keeps the
 * refusal point, the single host synchronisation and the batching guarantee of mml_world_map_add, now over the moment bytes too,
 * and needs no scratch beyond the 52 bytes per point (0 new bytes per point; one float4 origin per slot in the call's table
 * block).  _reset of one map carries the other maps' moments over.  The arithmetic, csrc/world_map_key.h (host and device):
 *   voxel centre  per axis c = ((float)i + 0.5f) * leaf in float, i the voxel index; offset d = w - c in float, w the world point;
 *   view vector   v = o - w per axis in float, o = ((float)T[3], (float)T[7], (float)T[11]) the sensor origin of the point's slot;
 *   moments       12 floats, three float4: (sdx, sdy, sdz, vx) (sxx, sxy, sxz, vy) (syy, syz, szz, vz).  One point: sd += d per
 *                 axis; the six products dx*dx, dx*dy, dx*dz, dy*dy, dy*dz, dz*dz, each rounded to float and then added; v +=
 *                 v_point per axis.  The points of a voxel in the order of the sums (call, slot, fused point order), each add
 *                 starting from the stored value;
 *   covariance    of a voxel of n >= 3 points, in double: nd = (double)n, m_a = (double)sd_a / nd, C_ab = (double)s_ab / nd -
 *                 m_a * m_b; Eigen's 3x3 self-adjoint solver as restated in csrc/eig3_dev.h (what mml_model_fit5's MML_FIT_EIG3
 *                 runs) on m00 = Cxx, m10 = Cxy, m11 = Cyy, m20 = Cxz, m21 = Cyz, m22 = Czz;
 *   surfel        8 floats: nx ny nz = (float) of the eigenvector of ev[0] as the solver returns it, all three components negated
 *                 when (n.x*V.x + n.y*V.y) + n.z*V.z < 0 -- the dot product in double of the solver's vector and the stored view
 *                 sum V; a dot of exactly 0 leaves the vector as it is --; l0 l1 l2 = (float)ev[0..2], ascending, as computed
 *                 (values slightly below 0 from rounding are reported, not clamped); planarity = (float)((ev1 - ev0) / ev2) and
 *                 linearity = (float)((ev2 - ev1) / ev2), in double, both 0 when ev2 <= 0.  A voxel of n < 3 points: eight zeros.
 * mml_world_map_download_moments: the raw accumulators, 12 floats per voxel in the order above -- what an NDT or GICP user
 * builds a covariance from.  mml_world_map_download_surfels: the 8-float records, one lane per voxel.  Both return the voxels in
 * the ascending key order of mml_world_map_download (row i of all three is the same voxel) through the same collect, sort and
 * gather chain; out == NULL is the sizing call; MML_ERR_CAPACITY when `capacity` (voxels) is below the count; MML_ERR_STATE,
 * naming the flag, on a map created without MML_WM_SURFELS; MML_ERR_INVALID for a NULL context, a NULL n_voxels or a map outside
 * [0, n_maps). */
#define MML_WM_SURFELS 1u
int mml_world_map_create_opts(mml_ctx* ctx, int n_maps /* 1..1024 */, float leaf, long capacity_voxels, unsigned flags);
int mml_world_map_download_moments(mml_ctx* ctx, int map, float* out /* n x 12 */, long capacity, long* n_voxels);
int mml_world_map_download_surfels(mml_ctx* ctx, int map, float* out /* n x 8 */, long capacity, long* n_voxels);

/* The feature node's own output: the six PointXYZINormal clouds of one union_cloud message (union-cloud/msg/union_cloud.msg:4-9)
 * for `count` extracted slots.  Cloud index k, in the message's order: 0 velo_corner, 1 velo_surface, 2 velo_combine,
 * 3 livox_corner, 4 livox_surface, 5 livox_combine.  Records are the 48-byte records of mml_scan_download_pointxyzinormal
 * (same fields, same padding); `out` is slot-major, then k, contiguous: cloud (i, k) holds n_points[6 i + k] records and starts
 * at the sum of all earlier entries of n_points.  out == NULL: only n_points (count x 6) is filled -- the sizing call.
 *   k = 2, 5: byte for byte the records mml_scan_download_pointxyzinormal returns for the slot, split at the Velodyne count;
 *       the Livox part as it stands (under the extrinsic when mml_extract was given one or a refresh applied one,
 *       unionFeatureExtract.cpp:312-318).
 *   k = 0, 1: the Velodyne points labelled 1 / 2, in the order of the sensor's RAW cloud (:1244-1252), cropped near and far
 *       (:1287-1295), with the sensor's intensity (velo_combine carries 0, :1254-1256); normal_x = in-sweep time, normal_y = ring,
 *       normal_z = label.  n_points = velo_corner_num, velo_surf_num of mml_scan_info_get.
 *   k = 3, 4: the Livox points labelled 1 / 2 in raw order -- of the cloud left by the `line > 5` / `x < 0.01` drops, :985-998 --,
 *       cropped near ONLY (:925, :933): they include the labelled points beyond far_th, which are in no other output; never
 *       under the extrinsic (the reference transforms livox_combine alone).  n_points = livox_corner_num, livox_surf_num.
 * Belongs between mml_extract and mml_undistort, like mml_gicp_refresh: MML_ERR_STATE for a slot that holds an uploaded
 * (mml_cloud_upload) or an undistorted cloud, or whose raw scan was uploaded again since its extraction (the raw order is read
 * from the raw records).  MML_ERR_CAPACITY, before any record is written, when capacity_points is below the total;
 * MML_ERR_INVALID for a slot range outside the context, count < 1 (or above 65535) or NULL n_points.  Nothing in the slots is
 * modified.  TWO host synchronisations whatever `count` is (counters and flags; records), one for the sizing call. */
int mml_feature_clouds_download_batch(mml_ctx* ctx, int first_slot, int count, uint8_t* out, long capacity_points,
                                      int* n_points /* count x 6 */);
/* One slot: the count = 1 case of the batch call (the same code path). */
int mml_feature_clouds_download(mml_ctx* ctx, int slot, uint8_t* out, int capacity_points, int* n_points /* 6 */);

/* ---- the aligner's time-offset search ---------------------------
 * The numeric core of LidarsParamEstimator::estimate_timeoffset (unionLidarsAligner.cpp:1077-1153): the Velodyne
 * cloud (n_velo x 3 floats) goes through pcl::transformPointCloud with tf (row-major 4x4 floats, NULL = identity;
 * _velo_hori_tf_matrix, :1080-1082); every Livox point (n_livox x 3 floats, the merged last eight messages in arrival
 * order, :1053-1068) gets the squared distance to its nearest transformed Velodyne point (:1084-1103, exact, on the
 * device grid that serves the association); window cnt sums dis_errors[i] + 0.2 * sqrt(x_i^2 + y_i^2) over
 * i in [cnt * search_resolution, cnt * search_resolution + sliced_points) while that end stays below n_livox (:1111-1131).
 * Outputs: nn_d2 (optional, n_livox floats), window_error (optional, `capacity` doubles), *n_windows, *best_window =
 * the window of the first strict minimum below 1e6 (-1: none) and *lowest_error (:1107,1141-1150).  n_velo must not
 * exceed max_map_points.  The caller turns best_window into a stamp (:1143) and applies _time_esti_error_th (:1155). */
int mml_time_offset_search(mml_ctx* ctx, const float* velo_xyz, int n_velo, const float* tf, const float* livox_xyz,
                           int n_livox, int search_resolution, int sliced_points, float* nn_d2, double* window_error,
                           int capacity, int* n_windows, int* best_window, double* lowest_error);
/* The search above for n problems in one device call.  Problem i: rows velo_offsets[i] .. velo_offsets[i+1]-1 of velo_xyz
 * (transformed with the matrix tf + 16 i; tf == NULL: no problem is transformed) are searched from rows livox_offsets[i] ..
 * livox_offsets[i+1]-1 of livox_xyz.  Every output of problem i is what mml_time_offset_search returns for that problem alone, to
 * the byte: n_windows[i], best_window[i], lowest_error[i], the rows livox_offsets[i] .. of nn_d2 (optional; indexed like
 * livox_xyz) and the window errors, written at window_error + window_offsets[i] -- at most window_offsets[i+1] - window_offsets[i]
 * of them, the single call's `capacity` rule (window_error is optional; window_offsets is read only with it).  A problem
 * without Livox points yields 0 windows, -1 and 1e6; one with no more than sliced_points Livox points yields 0 windows and its
 * nn_d2 rows.  All problems are checked before any device work and a refusal writes nothing: MML_ERR_INVALID for n outside
 * 1 .. MML_TOFS_BATCH_MAX, negative or decreasing offsets, a NULL required pointer, search_resolution or sliced_points below 1,
 * a problem with Livox points and no Velodyne point; MML_ERR_CAPACITY for a Velodyne cloud above max_map_points;
 * mml_last_error names the entry point and, where there is one, the problem.
 * Host synchronisations: the call first waits for everything the context has in flight, then synchronises exactly TWICE whatever
 * n is -- after the read-back of the n bounding boxes, from which the host lays out every problem's grid in one pass, and after
 * the read-back of the results (none when the call holds no Livox point at all).  With profiling on, each of the two phases
 * shows as one launch of the stages "tofs_box" and "tofs_search" per call.
 * The context keeps one grow-only scratch block for the largest call it has seen (100 bytes per Velodyne point -- the grid cells,
 * 8 per point, included --, 16 per Livox point, 8 per window, the sort's scratch), released by mml_destroy; MML_ERR_HIP, before
 * any launch, when it cannot be grown.  mml_time_offset_search is the n = 1 case of the same code and uses the same block.
 * MML_TOFS_BATCH_MAX bounds n because the problem index is a grid's y dimension. */
#define MML_TOFS_BATCH_MAX 65535   /* problems per call */
int mml_time_offset_search_batch(mml_ctx* ctx, int n,
        const float* velo_xyz, const int* velo_offsets /* n + 1 */,
        const float* tf /* n x 16, or NULL = identity for every problem */,
        const float* livox_xyz, const int* livox_offsets /* n + 1 */,
        int search_resolution, int sliced_points,
        float* nn_d2 /* livox_offsets[n] floats, may be NULL */,
        double* window_error /* may be NULL */, const long* window_offsets /* n + 1, required iff window_error */,
        int* n_windows /* n */, int* best_window /* n */, double* lowest_error /* n */);
/* The checks of the batch call that need no device, on the host alone (no context): the return code the call would refuse the
 * offsets and parameters with (max_map_points < 0: no capacity check), *bad_problem (optional) = the problem a refusal is
 * about or -1, and -- only with MML_OK -- n_windows[i] (optional) = (n_livox_i - sliced_points - 1) / search_resolution + 1
 * when n_livox_i > sliced_points, else 0. */
int mml_time_offset_plan(int n, const int* velo_offsets, const int* livox_offsets, int search_resolution, int sliced_points,
                         int max_map_points, int* n_windows /* n, may be NULL */, int* bad_problem /* may be NULL */);

/* ---- the aligner's Velodyne field-of-view selection: the input of the time-offset search ---------------------------------
 * velo_cloud_handler (unionLidarsAligner.cpp:437-490) for n Velodyne frames in one call: per point ori = -atan2f(y, x), unwrapped
 * along the sweep by the halfPassed state machine (:461-477), relTime = (ori - startOri) / (endOri - startOri) (:479), and the
 * point is kept iff ori lies in (-0.7608, 0.7158) or in that interval + 2 pi (:482-483).  The kept points of a frame, in input
 * order, are velo_fovs_cloud: what :511 queues, :674 / :1080 hand to estimate_timeoffset and :603-609 publish as velo_inFOV.
 * The arithmetic is the reference's to the bit (float / double mix as written, glibc's atan2f; csrc/velo_fov.h).
 * Input, PointCloud2-style as in mml_scan_upload_pointcloud2: frame i is n_points[i] records of point_step bytes at
 * data + byte_offsets[i] with float32 fields at off_x / off_y / off_z (packed x, y, z, intensity rows: point_step 16, offsets
 * 0, 4, 8) -- the payload velo_cloud_handler receives.  Frames may lie anywhere in `data`, overlap or repeat.
 * Output: the kept rows of frame i start at row n_kept[0] + ... + n_kept[i-1] of xyzt (x, y, z, relTime) and of xyz (x, y, z);
 * either may be NULL.  xyz is the velo_xyz of mml_time_offset_search_batch and the running sums of n_kept are its velo_offsets.
 * With both NULL the call is the sizing call (n_kept and info only; capacity_rows is not read).  info (optional) gives per frame
 * startOri, endOri, h = the point that set halfPassed (-1: none did) and n_kept.  A frame of 0 points (where the reference reads
 * points[0]) keeps nothing: info 0, 0, -1, 0.  A point with a NaN / Inf azimuth is never kept and never sets halfPassed.  A NaN
 * first (last) point makes startOri (endOri) and every relTime NaN and switches the unwrapping that compares against it off; the
 * predicate still reads ori alone, so such a frame keeps points by their unadjusted azimuth, as the reference's statements do.
 * Checks, all before any device work, and a refusal writes nothing: MML_ERR_INVALID for n outside 1 .. MML_FOV_BATCH_MAX, a NULL
 * byte_offsets / n_points / n_kept (or data with points to read), a negative count, offset or capacity_rows, point_step < 12, a
 * field offset outside [0, point_step - 4] or not 4-byte aligned; MML_ERR_CAPACITY for a frame above max_velo_points (with a
 * context only).  MML_ERR_CAPACITY also when capacity_rows is below the total kept: no row, count or info is then written.
 * mml_last_error names the entry point and, where there is one, the frame.
 * ctx == NULL runs the same routine on the host, frame after frame, and equals the device path to the byte: rows, counts, info.
 * With a context: one workgroup per frame (MML_FOV_BATCH_MAX bounds n because the frame index is a grid's y dimension), two
 * launches and at most TWO host synchronisations whatever n is -- after the read-back of counts and info, and after the
 * read-back of the rows (the sizing call and a call that keeps nothing: one).  With profiling on each of the two shows as one
 * launch of the stage "velo_fov".  Frames of up to 4096 points stay in registers between the phases; larger ones (any size up to
 * max_velo_points) park one float per point in scratch.  The context keeps one grow-only scratch set for the largest call it has
 * seen -- per input point point_step + 48 bytes on the device and point_step pinned, per frame 48 of each --, released by
 * mml_destroy; MML_ERR_HIP, before any launch, when it cannot be grown.  mml_velo_fov_select is the n = 1 case of the same code. */
#define MML_FOV_BATCH_MAX 65535   /* frames per call */
typedef struct { float start_ori, end_ori; int half_index /* h, -1: never */; int n_kept; } mml_velo_fov_info;
int mml_velo_fov_select_batch(mml_ctx* ctx /* NULL: the host build of the same routine */, int n,
        const uint8_t* data, const long* byte_offsets /* n */, const int* n_points /* n */,
        int point_step, int off_x, int off_y, int off_z,
        float* xyzt /* kept rows x,y,z,relTime; may be NULL */, float* xyz /* packed x,y,z; may be NULL */,
        long capacity_rows, int* n_kept /* n */, mml_velo_fov_info* info /* n, may be NULL */);
int mml_velo_fov_select(mml_ctx* ctx, const uint8_t* data, int n_points, int point_step, int off_x, int off_y, int off_z,
        float* xyzt, float* xyz, int capacity_rows, int* n_kept, mml_velo_fov_info* info);   /* n = 1, same code path */

/* ---- the aligner node's frame assembly: a Livox point stream cut into scan slots ----------------------------------------
 * The steady-state work of unionLidarsAligner.cpp on the device.  A mml_livox_stream is the aligner's point queue
 * (_hori_points_queue / _hori_points_stamp_queue) in device memory: a flat array of 20-byte records and a flat array of
 * 64-bit stamps.  mml_livox_stream_push is transform_hori_timestamp (:736-763) for one message: hs is the time base of the
 * first message pushed since creation or reset (_hori_start_stamp, :203-207) and point j gets the stamp
 * S = (timebase - hs) + offset_time, in nanoseconds.  Points are counted absolutely over everything ever pushed: `front` is
 * the queue's first point, `tail` one past its last.
 * Push: one host-to-device copy and one kernel, asynchronous on the context's stream (the host buffer must stay valid until
 * the next synchronising call); the wire form takes the 19-byte records of mml_scan_upload_wire and decodes them on the
 * device.  MML_ERR_CAPACITY, changing nothing, when the live points (tail - front) plus n exceed capacity_points.  When the
 * array's end is reached the live part moves to the front of a second array of the same size (one device-to-device copy on
 * the stream, no host synchronisation; the two arrays never overlap), so a stream holds 56 bytes per point of capacity, plus
 * 19 for the wire staging once push_wire has been used.
 * TIME ORDER.  The frame cut below needs hs + S[i] >= hs + S[i-1] for every point, across messages too (the reference's own
 * comment at :738 intends that; what it does with unordered stamps depends on the order of its walk and is not reproduced).
 * The push kernel counts the violations (`disorder`); mml_union_assemble refuses a stream that has any.
 * A stream belongs to its context and must be destroyed before it.  mml_livox_stream_reset empties it and forgets hs and
 * the violations. */
typedef struct mml_livox_stream mml_livox_stream;
int  mml_livox_stream_create(mml_ctx* ctx, long capacity_points, mml_livox_stream** out);
void mml_livox_stream_destroy(mml_livox_stream* s);
int  mml_livox_stream_reset(mml_livox_stream* s);
int  mml_livox_stream_push(mml_livox_stream* s, uint64_t timebase, const mml_livox_point* pts, int n);
int  mml_livox_stream_push_wire(mml_livox_stream* s, uint64_t timebase, const uint8_t* wire, int n);
typedef struct { uint64_t start_stamp; long front, tail; long disorder; } mml_livox_stream_state;
/* hs (0 before the first push), front, tail and the violations counted so far; synchronises the context's stream. */
int  mml_livox_stream_state_get(mml_livox_stream* s, mml_livox_stream_state* out);

/* pub_horipoints_given_stamp (:766-868) and the union_cloud assembly of :343-364 for `count` consecutive Velodyne frames in
 * one call.  Frame i is [stamps[i], stamps[i+1]) in absolute nanoseconds (the Velodyne header stamps, :343-344) and fills
 * slot first_slot + i:
 *   Velodyne part: rows velo_offsets[i] .. velo_offsets[i+1]-1 of velo_xyzi (x, y, z, intensity floats) through
 *     pcl::transformPointCloud with tf (row-major 4 x 4 floats, _velo_hori_tf_matrix, :352; NULL: copied), in float,
 *     t0 * x + t1 * y + t2 * z + t3 summed left to right, the intensity carried;
 *   Livox part: the points [begin, end) of the stream, x, y, z, reflectivity, tag, line unchanged, _pad = 0 and
 *     offset_time = (uint32)(hs + S[k] - stamps[i]), the truncating assignment of :823.
 * With q the front and A[k] = hs + S[k]:  q == tail: EMPTY (:769-773).  A[q] >= start: begin = q and the gate is A[q];
 * otherwise the walk of :789-800 ends one past its first match j (the first point at or after q with A[j] >= start):
 * begin = j + 1 and the gate is A[j]; NOT_REACHED when there is no such j.  The gate, not the stamp of point `begin`, decides
 * whether `begin` goes out (:811); after it k = begin + 1 ... goes out while k < tail and A[k] < end.  OK moves the front to
 * max(q, end - 100) (:862-863); every status but OK and OVERFLOW leaves it.
 * Where the reference is undefined this library defines: a gate at or after `end`, or begin == tail, emits nothing (the
 * reference then reads front() of an empty vector, :842): NO_POINTS; the read of the stamp one past the last point (:837) ends
 * the loop; the negative erase count of :862 for end - q < 100 erases nothing.  A frame of more than max_livox_points
 * points is OVERFLOW: the slot gets no Livox point, n_livox reports the count that was needed, and the front moves as for OK,
 * so that the frames after it are what they would have been.
 * Rows of frames that emit nothing have n_livox = 0, front_after = q and begin = end = the `begin` above where it exists
 * (NO_POINTS), else q.  A frame whose status is not OK still gets its Velodyne part, with zero Livox points.
 * Afterwards every slot of the call is in the state mml_scan_upload leaves it in (device and host counts set, the extracted
 * state invalidated), so mml_extract follows.  count frames in one call equal count calls of one frame, to the byte: slots,
 * rows and the stream afterwards.
 * Everything is checked before any device work and a refusal writes nothing: MML_ERR_INVALID for a slot range outside the
 * context, count outside 1 .. MML_UNION_BATCH_MAX, a NULL stream / stamps / velo_offsets / out (or velo_xyzi with rows to
 * copy), a stream of another context, decreasing stamps or velo_offsets or a negative velo_offsets[0]; MML_ERR_CAPACITY for
 * a frame with more than max_velo_points Velodyne rows.  MML_ERR_STATE, from the call's one read-back, for a stream with
 * time-order violations: the kernels have then written neither slots nor counts, and the rows are not written either.
 * Host synchronisations: ONE whatever count is -- the read-back of the count rows together with the violation counter,
 * after which the host advances its copy of the front.  Two kernel launches per call whatever count is, which profiling shows
 * as one launch each of the stages "union_plan" (count + 1 binary searches over the live stamps, then the front's
 * recurrence by one lane out of LDS, the rows and the slots' counts) and "union_gather" (the Livox records as a dword
 * stream, the Velodyne transform).  The context keeps one grow-only staging block (16 bytes per Velodyne row of the largest
 * call, 56 per frame), released by mml_destroy. */
typedef struct { int status; int n_livox; long begin, end; long front_after; } mml_union_frame;
/* status: 0 OK, 1 EMPTY, 2 NOT_REACHED, 3 NO_POINTS, 4 OVERFLOW */
#define MML_UNION_BATCH_MAX 65535   /* frames per call: the frame index is a grid's y dimension */
int mml_union_assemble(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count,
                       const uint64_t* stamps /* count + 1: frame i = [stamps[i], stamps[i+1]) */,
                       const float* velo_xyzi, const int* velo_offsets /* count + 1 */,
                       const float* tf /* 16 or NULL */, mml_union_frame* out /* count */);
/* Host only, no context: the rows mml_union_assemble returns for a stream whose stamps are the host array S, indexed
 * absolutely (S[front] .. S[tail-1] are read).  MML_ERR_INVALID for count outside 1 .. MML_UNION_BATCH_MAX, a NULL pointer,
 * front < 0 or tail < front, decreasing stamps; MML_ERR_STATE for a time-order violation in [front, tail). */
int mml_union_plan(const uint64_t* S, long front, long tail, uint64_t hs, int count, const uint64_t* stamps,
                   int max_livox_points, mml_union_frame* out);

/* The aligner's OTHER live mode: once the time offset is known -- estimated by mml_time_offset_search (:1161) or given
 * (:178-184) -- velo_cloud_handler (:513-551) calls the one-stamp overload pub_horipoints_given_stamp(start_stamp, msg)
 * (:872-1009), which cuts a fixed COUNT of points instead of an interval.  This is that overload for `count` Velodyne frames in
 * one call, on the same stream.  Frame i has the stamp t = starts[i] (absolute ns: the Velodyne header stamp minus the time
 * offset, formed by the caller in uint64 as :520 does), c = sliced_points (_offset_search_sliced_points) and fills slot
 * first_slot + i.  With q the front, T the tail and A[k] = hs + S[k]:
 *   q == T: EMPTY (:874-878), the front stays.
 *   The walk of :896-918 erases front points while A[front] < t and more than one point is queued.  Let L be the first k in
 *   [q, T) with A[k] >= t, else T.  L < T: the front becomes L.  L == T: the walk stops with one point left and returns false:
 *   NOT_REACHED -- and, unlike in mml_union_assemble, the queue HAS changed: front_after = T - 1, begin = end = T - 1,
 *   n_livox = 0.
 *   n = min(c, T - L) >= 1 points L .. L + n - 1 go out (:946-980): x, y, z, reflectivity, tag, line unchanged, _pad = 0,
 *   offset_time = (uint32)(A[k] - t), the truncating assignment of :955/:964.  All of them are erased: OK, begin = L,
 *   end = front_after = L + n.  There is no keep-100 in this overload.
 *   Velodyne part: exactly that of mml_union_assemble (tf is _velo_hori_tf_matrix, :528); a frame whose status is not OK still
 *   gets it, with zero Livox points.
 * The overload has no undefined read (the front() at :912 and :984 always has an element), so there is no NO_POINTS, and no
 * OVERFLOW: sliced_points > max_livox_points is refused.  Which Velodyne frame goes with which cut is the caller's business:
 * rows velo_offsets[i] .. pair with starts[i] (the reference's own handler erases its Velodyne queue twice, :1005 and :543;
 * see INTEGRATION.md).
 * Slots afterwards, batch equivalence (count frames in one call equal count calls of one frame to the byte, in slots, rows and
 * the stream afterwards), the checks before any device work and MML_ERR_STATE are those of mml_union_assemble, with `starts`
 * (count entries, must not decrease) in the place of `stamps`; in addition MML_ERR_INVALID for sliced_points < 1 and
 * MML_ERR_CAPACITY for sliced_points > max_livox_points.  The two assemble calls may be mixed on one stream.
 * ONE host synchronisation and two kernel launches per call whatever count is: the stages "union_offset_plan" (count binary
 * searches, the recurrence q' = min(max(q, L_i) + c, T) -- T - 1 for NOT_REACHED -- by one lane out of LDS, the rows and the
 * slots' counts) and "union_gather" (the kernel of mml_union_assemble, unchanged).  The host front advances to the last row's
 * front_after, which moves for NOT_REACHED too.  Staging is shared with mml_union_assemble. */
int mml_union_assemble_offset(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count,
                              const uint64_t* starts /* count, absolute ns, must not decrease */, int sliced_points,
                              const float* velo_xyzi, const int* velo_offsets /* count + 1 */,
                              const float* tf /* 16 or NULL */, mml_union_frame* out /* count */);
/* Host only, no context: the rows mml_union_assemble_offset returns for the host stamp array S (as mml_union_plan reads it).
 * MML_ERR_INVALID for count outside 1 .. MML_UNION_BATCH_MAX, a NULL pointer, front < 0 or tail < front, decreasing starts,
 * sliced_points < 1; MML_ERR_STATE for a time-order violation in [front, tail). */
int mml_union_plan_offset(const uint64_t* S, long front, long tail, uint64_t hs, int count, const uint64_t* starts,
                          int sliced_points, mml_union_frame* out);

/* ---- the aligner's time-offset estimation on the resident stream -------------------------------------------------------
 * LidarsParamEstimator::estimate_timeoffset (unionLidarsAligner.cpp:1021-1166) for n queued Velodyne frames against one range of
 * a mml_livox_stream, in one call and without a hand-over through host memory: frame i (a PointCloud2-style payload, the
 * arguments of mml_velo_fov_select_batch) goes through the FOV selection of :437-490; its kept points, transformed by tf (ONE
 * row-major 4 x 4 matrix for all frames, _velo_hori_tf_matrix; NULL: not transformed), are searched from the stream's points
 * [livox_begin, livox_end) -- absolute point indices with front <= livox_begin <= livox_end <= tail, the merged last eight
 * messages of :1049-1074, whose boundaries the caller knows from its pushes.  All frames share that one Livox block.
 * Every numeric output of row i -- n_kept, n_windows, best_window, lowest_error, row i of nn_d2 (livox_end - livox_begin floats
 * per frame; optional) and the window errors at window_error + window_offsets[i], at most window_offsets[i+1] -
 * window_offsets[i] of them (optional; the batch call's capacity rule) -- equals, to the byte, mml_velo_fov_select_batch of the
 * frame followed by mml_time_offset_search of its xyz rows against the x, y, z of the same records.
 * optim_start = hs + S[livox_begin + best_window * search_resolution], the stream's own stamp of the best window's first point,
 * which is livox_msg.timebase + livox_msg_offset_vec[cnt * search_res] of :1146 (hs + S[k] = the time base of k's message + its
 * offset_time).  time_offset = velo_stamps[i] - optim_start in uint64 (:1161; it wraps when the Livox clock is ahead).  accepted =
 * best_window >= 0 && lowest_error < error_th (:1159).  Without a best window the three are 0.
 * The stream is only read: front, tail, disorder and every record stay, so mml_union_assemble_offset can follow on it.  A stream
 * with time-order violations is not refused: the search does not depend on the order.
 * Checks, all before anything is enqueued, and a refusal writes nothing: MML_ERR_INVALID for the argument rules of
 * mml_velo_fov_select_batch, n outside 1 .. min(MML_FOV_BATCH_MAX, MML_TOFS_BATCH_MAX), a range outside [front, tail] or
 * reversed, a stream of another context, search_resolution or sliced_points below 1, a NULL stream / velo_stamps / out (or
 * window_offsets with window_error), negative or decreasing window_offsets; MML_ERR_CAPACITY for a frame above max_velo_points,
 * for a frame above max_map_points -- deliberately conservative: the frame's POINTS are counted, not the ones it will keep, which
 * only the device knows -- and for n x (livox_end - livox_begin) or the frames' points together above INT_MAX.  mml_last_error
 * names the entry point and, where there is one, the frame.
 * The one condition known only on the device: a frame that keeps nothing while the range holds points.  The hand-composed path
 * refuses such a problem up front (mml_time_offset_search: "nearest-neighbour search in an empty cloud"); here it is that row's
 * status NO_VELO_IN_FOV with 0 windows, -1 and 1e6, its nn_d2 row and window errors are left unwritten, and the other frames
 * are unaffected.
 * On the device: one upload of the payload; the FOV kernel's rows are packed straight into the search's Velodyne input (no row
 * crosses the bus, the counts do); k_tofs_livox_xyz forms the packed x, y, z of the range from the stream's records; the
 * kernels of mml_time_offset_search_batch do the rest, and k_tofs_rows reads S for the best windows and writes the rows.
 * Host synchronisations: the call first waits for everything the context has in flight, then synchronises exactly THREE times
 * whatever n is -- the FOV counts, the bounding boxes, the results -- (ONE, the counts, for an empty range or when no frame keeps a
 * point).  With profiling on they show as one launch each of the stages "velo_fov", "tofs_box" and "tofs_search" per call.
 * Scratch: the grow-only blocks of mml_velo_fov_select_batch and mml_time_offset_search_batch (4 n (livox_end - livox_begin)
 * bytes of distances among them). */
typedef struct {
    int status;            /* 0 OK, 1 NO_VELO_IN_FOV (the frame kept nothing while the range holds points) */
    int n_kept;            /* velo_fovs_cloud size of the frame */
    int n_windows, best_window;      /* as mml_time_offset_search */
    double lowest_error;
    uint64_t optim_start;  /* hs + S[livox_begin + best_window * search_resolution]; 0 when best_window < 0 */
    uint64_t time_offset;  /* velo_stamps[i] - optim_start in uint64 (:1161); 0 when best_window < 0 */
    int accepted;          /* best_window >= 0 && lowest_error < error_th (:1159) */
    int _pad;
} mml_time_offset_estimate_row;
#define MML_TOFS_ROW_OK 0
#define MML_TOFS_ROW_NO_VELO_IN_FOV 1
int mml_time_offset_estimate_stream(mml_ctx* ctx, mml_livox_stream* s, long livox_begin, long livox_end,
        int n, const uint8_t* data, const long* byte_offsets /* n */, const int* n_points /* n */,
        int point_step, int off_x, int off_y, int off_z,
        const uint64_t* velo_stamps /* n, header stamps in ns */, const float* tf /* 16 or NULL */,
        int search_resolution, int sliced_points, double error_th,
        float* nn_d2 /* n x (livox_end - livox_begin), may be NULL */,
        double* window_error /* may be NULL */, const long* window_offsets /* n + 1, required iff window_error */,
        mml_time_offset_estimate_row* out /* n */);
/* Host only, no context: which queued Velodyne frame estimate_timeoffset runs on -- the loop of :1026-1043.  velo_stamps: the
 * header stamps (ns) of the n_velo queued frames, oldest first (velo_vec); hori_stamp: the header stamp of the newest Livox
 * message (hori_vec.back(), :1027); n_hori_msgs: hori_vec.size().  From the newest frame backwards a frame is popped while it
 * is newer than hori_stamp or within 0.2 s of it, stamps compared as ros::Time::toSec() forms them ((double)sec + 1e-9 *
 * (double)nsec from ns / 1000000000 and ns % 1000000000) and `abs` being std::abs(double) (convention 15).
 * *selected = the index of the frame :1044 ends on, *status = MML_TOFS_GATE_OK.  Where the reference is undefined this library
 * refuses and selects nothing (*selected = -1): MML_TOFS_GATE_EMPTY when every frame is popped (the reference pops its last
 * frame and reads back() of an empty vector, :1037-1039; n_velo == 0 likewise), MML_TOFS_GATE_TOO_FEW_MESSAGES when a frame is
 * left but n_hori_msgs < 8 (:1051 indexes before the vector's start).  Returns MML_OK, or MML_ERR_INVALID for a negative count
 * or a NULL pointer. */
#define MML_TOFS_GATE_OK 0
#define MML_TOFS_GATE_EMPTY 1
#define MML_TOFS_GATE_TOO_FEW_MESSAGES 2
int mml_time_offset_gate(int n_velo, const uint64_t* velo_stamps, uint64_t hori_stamp, int n_hori_msgs,
                         int* selected /* index of the frame :1044 ends on, or -1 */, int* status);

/* Test hook like mml_libm_f32: a slot's raw input as it stands -- what the upload entry points or mml_union_assemble put
 * there: n_velo rows of x, y, z, intensity and n_livox records.  Either buffer may be NULL with capacity 0 to query the
 * counts; MML_ERR_CAPACITY when a capacity is below its count.  Synchronises. */
int mml_scan_raw_download(mml_ctx* ctx, int slot, float* velo_xyzi, int cap_velo, mml_livox_point* livox, int cap_livox,
                          int* n_velo, int* n_livox);

/* ---- SURVEY section 8(f) rank 4 (the other part): the per-frame GICP extrinsic refresh ---------------------------------
 * icp_ext_matching (unionFeatureExtract.cpp:74-123): pcl::GeneralizedIterativeClosestPoint with setMaximumIterations(10),
 * setTransformationEpsilon(1e-6), PCL defaults otherwise, identity guess -- the published PCL 1.8.1 algorithm (20-NN
 * covariances regularised to (1, 1, 1e-3), 1-NN correspondences, BFGS over (t, roll, pitch, yaw) with the float
 * transformation of applyState), all on the device.  src / tgt: n x 3 floats.  T_inout (row-major 4 x 4 float) is
 * overwritten with getFinalTransformation() only when *converged = 1 (hasConverged(), :91-96); clouds with fewer than 20
 * points or fewer than 4 correspondences do not converge ("ICP Failed", :119-122). */
typedef struct {
    int outer_iterations;        /* nr_iterations_ */
    int objective_evaluations;   /* BFGS function / gradient evaluations over all outer iterations */
    double objective;            /* f at the end of the last inner minimisation */
    int n_source, n_target;
} mml_gicp_info;
int mml_gicp_align(mml_ctx* ctx, const float* src_xyz, int n_src, const float* tgt_xyz, int n_tgt, float* T_inout, int* converged,
                   mml_gicp_info* info /* may be NULL */);
/* The call site, unionCloudHandler (:302-318), on a slot that mml_extract filled WITHOUT an extrinsic: when
 * livox_corner_num > 100 the slot's Livox surf cloud (source) is aligned to its Velodyne surf cloud (target) -- every
 * frame, _extrin_cnt never advances (:199,307) -- extrinsic_inout = extri_mtx is updated if the alignment converged
 * (*refreshed), and with apply != 0 the Livox part of the fused cloud is transformed with the (updated or kept) matrix
 * (pcl::transformPointCloud, :312).  With livox_corner_num <= 100 nothing happens, as in the reference.  The two surf
 * clouds are the reference's: label-2 points in the order of each sensor's raw cloud (:1024-1031, :1242-1252), the
 * Velodyne one cropped near + far (:1287-1293), the Livox one near only (removeNearPointCloud, :925 -- its labelled points
 * beyond far_th are part of the source although they are not part of the fused cloud).  MML_ERR_STATE when the slot holds
 * an uploaded or already undistorted cloud -- the refresh belongs between mml_extract and mml_undistort -- or when the slot's
 * raw scan was uploaded again after the extraction (the line ids of the raw records are re-derived from them).  Synchronous. */
int mml_gicp_refresh(mml_ctx* ctx, int slot, float* extrinsic_inout, int apply, int* refreshed, mml_gicp_info* info);
/* The two calls above for many problems in one device call.  The alignments of a call are independent (each starts from the
 * identity guess) and go through the same kernels as the single calls, one BFGS workgroup per problem: every T, converged and
 * info is what the single call returns for that problem alone, to the byte.  The context keeps one grow-only scratch block for
 * the largest call it has seen (88 bytes per surf point, 76 more per source point), released by mml_destroy; MML_ERR_HIP, before
 * any slot is touched, when it cannot be grown.
 * mml_gicp_align_batch: problem i is rows src_offsets[i] .. src_offsets[i+1]-1 of src_xyz against rows tgt_offsets[i] ..
 * tgt_offsets[i+1]-1 of tgt_xyz; T_inout + 16 i is its matrix (left alone unless converged[i]), a problem that does not align
 * (fewer than 20 points on a side) leaves converged[i] = 0 and info[i] zeroed.  MML_ERR_INVALID for n outside
 * 1 .. MML_GICP_BATCH_MAX, decreasing or negative offsets, a NULL pointer other than info.
 * mml_gicp_refresh_batch: slot first_slot + i is treated as mml_gicp_refresh treats it.  chain == 0: row i of extrinsics is slot
 * i's own matrix, in and out.  chain != 0: row 0 is the caller's persistent extri_mtx on entry (rows 1 .. are not read); on
 * return row i is the matrix held after frame i -- slot i's alignment if it converged, else what row i - 1 holds -- and it is
 * what is applied to slot i: a loop of mml_gicp_refresh over one matrix (the chain is run on the host between the result
 * read-back and the one apply launch).  All slots are checked before any device work; a refusal names the slot, returns the
 * single call's code (MML_ERR_INVALID for a range outside the context or count outside 1 .. MML_GICP_BATCH_MAX, MML_ERR_STATE
 * for a slot that is uploaded, undistorted or re-uploaded since its extraction) and changes no slot and no matrix.  Four host
 * synchronisations per call: slot states, surf counts, results, apply.  (The single calls are the n = 1 case of the same code;
 * mml_last_error names the entry point that was called.)  MML_GICP_BATCH_MAX bounds n and count because the problem index is
 * a grid's y dimension. */
#define MML_GICP_BATCH_MAX 65535   /* problems / slots per call */
int mml_gicp_align_batch(mml_ctx* ctx, int n, const float* src_xyz, const int* src_offsets /* n + 1 */,
                         const float* tgt_xyz, const int* tgt_offsets /* n + 1 */,
                         float* T_inout /* n x 16 */, int* converged /* n */, mml_gicp_info* info /* n, may be NULL */);
int mml_gicp_refresh_batch(mml_ctx* ctx, int first_slot, int count, float* extrinsics /* count x 16, in/out */, int chain,
                           int apply, int* refreshed /* count, may be NULL */, mml_gicp_info* info /* count, may be NULL */);
/* mml_gicp_align with the three settings the reference's call sites differ in as arguments.  The entry points above are the
 * call with {10, 1e-6, 0}, through the same kernels.  The gate is PCL 1.8.1's computeTransformation: a source point enters a
 * round's correspondence list iff its 1-NN squared distance (the float the search produces) is < the gate squared; a rejected
 * point contributes no term to the objective or its gradient and does not count in their 1/m, and fewer than 4 kept points end
 * the alignment unconverged with T_inout untouched, as too few points do.  The (correspondence, BFGS) rounds are enqueued in
 * chunks of at most ten with one read-back of the state per chunk, until the alignment has converged or failed: host
 * synchronisations = ceil(outer iterations run / 10), one for max_iterations <= 10.  MML_ERR_INVALID, before any device work,
 * for NULL opts, max_iterations < 1, a transformation_epsilon that is not finite and positive, a NaN gate. */
typedef struct {
    int    max_iterations;               /* setMaximumIterations */
    double transformation_epsilon;       /* setTransformationEpsilon */
    double max_correspondence_distance;  /* metres; <= 0: no gate (what mml_gicp_align does) */
} mml_gicp_opts;
int mml_gicp_align_opts(mml_ctx* ctx, const float* src_xyz, int n_src, const float* tgt_xyz, int n_tgt, const mml_gicp_opts* opts,
                        float* T_inout, int* converged, mml_gicp_info* info /* may be NULL */);

/* ---- the aligner node's start-up calibration (unionLidarsAligner.cpp:221-270, lidars_extrinsic_cali.h:493-618) -----------
 * mml_cloud_crop_voxel: removeFarPointCloud (lidars_extrinsic_cali.h:398-422) + pcl::VoxelGrid<PointXYZI> of a free cloud of
 * n x (x, y, z, intensity) floats, on the device.  A point is dropped iff (x*x + y*y) + z*z > far_th*far_th in float; order is
 * kept.  The filter is PCL 1.8.1's applyFilter with the conventions of mml_downsample: inverse leaf in float, floor of the
 * bounding box, voxel index i + j dx + k dx dy, output ascending by index, a voxel's points summed in input order in float and
 * divided by their number -- all four fields.  When the box holds more than INT32_MAX voxels (dx dy dz as int64, each
 * (int64)((max - min) * inverse_leaf) + 1) PCL refuses to filter: the output is then the cropped cloud, in input order, and
 * *unfiltered = 1.  out_xyzi == NULL: sizing call, *n_out and *unfiltered only.  MML_ERR_CAPACITY, before any record is written,
 * when capacity < *n_out (which is set); MML_ERR_INVALID for n < 0, a NULL cloud with n > 0, NULL n_out, far_th or leaf that
 * is not finite and positive.  One host synchronisation: the read-back of count and records in one copy.  The context keeps
 * grow-only scratch for the largest cloud it has seen (64 bytes per point on the device and the sort's temporary storage, 32
 * per point pinned), released by mml_destroy; MML_ERR_HIP, before any launch, when it cannot be grown. */
int mml_cloud_crop_voxel(mml_ctx* ctx, const float* xyzi, int n, float far_th, float leaf, float* out_xyzi, int capacity,
                         int* n_out, int* unfiltered /* may be NULL */);
/* calibratePCLICP and its call site: both clouds (source: the integrated Livox cloud _hori_igcloud, intensity = reflectivity;
 * target: _velo_new_cloud) through mml_cloud_crop_voxel's kernels with (50, 0.05), the filtered clouds staying on the device,
 * then mml_gicp_align_opts' with {500, 1e-3, 2.0} from the identity guess.  (setRANSACIterations(12) has no effect on PCL
 * 1.8.1's GICP: nothing is implemented for it.)  hori_tf = getFinalTransformation(); velo_hori_tf is what the caller makes
 * of it (:251-253): rows 0-2 are R^T and -t, row 3 is hori_tf's row 3 -- NOT the rigid inverse (that would be -R^T t); the
 * reference's matrix is reproduced as it is.  Both matrices are written only when *converged; fewer than 20 points left in a
 * cloud, or fewer than 4 correspondences inside the gate, do not converge.  Every result equals the three calls made one after
 * the other, to the byte.  Host synchronisations: 1 (the two filtered sizes) + ceil(outer iterations run / 10).
 * MML_ERR_INVALID for a negative count, a NULL cloud with points, NULL hori_tf, velo_hori_tf or converged. */
typedef struct {
    int n_hori_in, n_velo_in;              /* points handed in */
    int n_hori_ds, n_velo_ds;              /* after crop + voxel filter: what the alignment sees */
    int hori_unfiltered, velo_unfiltered;  /* PCL's overflow refusal hit: the cloud was cropped only */
    mml_gicp_info gicp;
} mml_calib_info;
int mml_aligner_calibrate(mml_ctx* ctx, const float* hori_xyzi, int n_hori, const float* velo_xyzi, int n_velo,
                          float* hori_tf /* 16 */, float* velo_hori_tf /* 16 */, int* converged, mml_calib_info* info /* may be NULL */);

/* ---- a1..a8: feature extraction -----------------------------------------------------------------
 * feature_extraction::unionCloudHandler minus the PCL GICP refresh (unionFeatureExtract.cpp:266-321):
 * getVeloFeature (:1113-1317) + getHoriFeature/getHoriFeatureExtract (:891-1035) with
 * detectFeaturePoints (:341-844) per ring / line, label scatter, near/far crop.  Result per slot: the
 * fused labelled cloud [velo_combine ; livox_combine] kept on the device (what PoseEstimation merges at
 * unionPoseEstimation.cpp:746-757).  livox_extrinsic: optional row-major 4x4 float applied to the Livox
 * part when livox_corner_num > 100 (:302-318); NULL = identity. */
int mml_extract(mml_ctx* ctx, int first_slot, int count, const float* livox_extrinsic);

typedef struct {
    int n_points;       /* fused cloud size */
    int n_velo;         /* leading points that came from the Velodyne */
    int velo_corner_num, velo_surf_num;   /* union_cloud.msg:16-19, set at :1299-1300 */
    int livox_corner_num, livox_surf_num; /* set at :939-940 */
    int fused_corner_num, fused_surf_num; /* label-1 / label-2 points of the fused cloud (corner_cnt, Estimator.cpp:990-1003) */
} mml_scan_info;
int mml_scan_info_get(mml_ctx* ctx, int slot, mml_scan_info* info);
/* Copies the fused labelled cloud of a slot to host (any pointer may be NULL).  Capacity must be
 * >= n_points.  label: 0 none / 1 corner / 2 surf (normal_z); line: ring or Livox line (normal_y);
 * reltime: normal_x.  xyzi: 4 floats per point. */
int mml_scan_download(mml_ctx* ctx, int slot, float* xyzi, float* reltime, uint8_t* line, uint8_t* label,
                      int capacity);

/* Unit-level twin of feature_extraction::detectFeaturePoints (unionFeatureExtract.cpp:341-343) for one
 * scan line: pts = n x (x,y,z,intensity) on the host; sharp / flat receive indices into the line
 * (capacity n each); flags (optional, n ints) receives CloudFeatureFlag[].  Runs in the buffers of scan slot 0:
 * whatever mml_extract / mml_cloud_upload left in slot 0 (fused cloud, labels, scan info) is invalid afterwards. */
int mml_detect_line(mml_ctx* ctx, const float* pts, int n, int* sharp, int* n_sharp, int* flat, int* n_flat,
                    int* flags);

/* ---- a9: RemoveLidarDistortion (unionPoseEstimation.cpp:402-421) ---------------------------------
 * In place on the fused cloud of each slot.  dR: count x 9, dt: count x 3 (host). Sets reltime to 1. */
int mml_undistort(mml_ctx* ctx, int first_slot, int count, const double* dR, const double* dt);

/* ---- a10: label split + pcl::VoxelGrid down-sample (Estimator.cpp:992-1026) ----------------------
 * Any number of labelled points per slot (up to 8192 per kind are sorted in LDS, denser clouds take a global-sort
 * path); the output stacks hold at most max_features voxels per kind (MML_ERR_CAPACITY at the next read-back
 * otherwise).  Not reproduced: PCL's refusal to filter when the voxel grid of a cloud has more than 2^31 cells (it
 * returns the input unfiltered; needs e.g. a 100 m cloud at 5 cm leaves). */
int mml_downsample(mml_ctx* ctx, int first_slot, int count);
/* kind: 0 corner (laserCloudCornerStack), 1 surf (laserCloudSurfStack). xyz: 3 floats per feature. */
int mml_features_download(mml_ctx* ctx, int slot, int kind, float* xyz, int capacity, int* n);
/* Test hook: replace the down-sampled stack of a slot with caller-provided features. */
int mml_features_upload(mml_ctx* ctx, int slot, int kind, const float* xyz, int n);

/* ---- a13 map side: laserCloud{Corner,Surf}FromLocal (Estimator.cpp:1159-1167) --------------------
 * Uploads a map cloud (3 floats per point) and builds the radix-sorted uniform grid that replaces
 * pcl::KdTreeFLANN::setInputCloud.  kind: 0 corner, 1 surf. */
int mml_map_set_local(mml_ctx* ctx, int kind, const float* xyz, int m);
/* ---- Estimator::MapIncrementLocal (Estimator.cpp:1585-1643), on the device ----------
 * Moves the down-sampled corner / surf stacks of `slot` (what mml_downsample left there) to the world frame with
 * T_wl = transformTobeMapped (row-major 4x4; pointAssociateToMap, Map_Manager.cpp:75-89), stores them in ring slot
 * localMapID % 50, rebuilds both local maps as pcl::VoxelGrid(concatenation of the ring) -- the clear() of
 * :1083-1085 / :1125-1127 included -- and rebuilds the kNN grids, all in HBM.  The caller keeps the key-scan rule
 * (pose moved by >= sqrt(0.5) m, :1082,1124).  n_*_map (optional) receive the new map sizes.
 * This is the n = 1 case of the chain mml_map_bank_increment_segmented runs for n banks (below), the two kinds its two
 * segments: both stacks are checked before any ring state changes (MML_ERR_STATE), and the call makes 2 + R host
 * synchronisations after its entry drain (the stack sizes; the filtered sizes and boxes; one per cell-refinement round, R =
 * the rounds of the slower kind, 1 to 5).  Memory, from the first increment on: the ring, 2 x 50 x max_features x 16
 * bytes, and the chain's scratch, which is shared with the banks and sized by need -- 48 bytes per ring point actually
 * held (both kinds, the new stacks included) plus the sort's temporary storage, grown on demand and kept until mml_destroy. */
int mml_map_increment_local(mml_ctx* ctx, int slot, const double* T_wl, int* n_corner_map, int* n_surf_map);
/* Empties the ring (localMapID = 0); the current local maps stay until the next set / increment. */
int mml_map_local_reset(mml_ctx* ctx);
/* Copies the current local map (as set or as rebuilt by mml_map_increment_local) to the host: 3 floats per point,
 * in the order the kNN indices refer to.  xyz may be NULL to query *n only. */
int mml_map_local_download(mml_ctx* ctx, int kind, float* xyz, int capacity, int* n);

/* ---- SURVEY section 8(f) rank 2, global half: the MAP_MANAGER cube stores on the device ----------------------------
 * mml_map_global_append   = MAP_MANAGER::featureAssociateToMap (Map_Manager.cpp:91-117): the down-sampled stacks of
 *                           `slot` moved to the world frame with T_wl and appended to the pending clouds
 *                           (laserCloud*_to_map of Estimator::threadMapIncrement, Estimator.cpp:120-122);
 * mml_map_global_increment = MAP_MANAGER::MapIncrement(pending, T_wl) (:125-281) incl. MapMove (:288-581): the cube
 *                           grid follows the sensor, new points go to their cubes, cubes that received points and hold
 *                           > 300 are voxel-filtered (leaf 0.4).  As in the reference (:136-149) the map Estimate()
 *                           matches against becomes the store as it was BEFORE this call (cubes, trees and centre):
 *                           the a12 grids and laserCloudCen*_last are rebuilt from it.  n_* (optional): live store
 *                           sizes after the update.
 * Both are the n-store chain of the map banks (mml_map_bank_global_*_segmented below) with n = 1 on the context's own store:
 * the same launches, 3 + R host synchronisations per increment, and the same refusals -- an append of a slot without a
 * down-sampled stack of EITHER kind (MML_ERR_STATE) or beyond 16 x max_features pending points (MML_ERR_CAPACITY), an increment
 * whose store would exceed max_map_points (MML_ERR_CAPACITY) or whose pose needs more than 64 layer shifts (MML_ERR_INVALID)
 * -- each of which leaves the store exactly as it was: live arrays, tags, centre, pending clouds, match copy.
 * Memory: the store's own arrays from the first append / increment on (72 bytes per point of max_map_points plus
 * 2 x 16 x max_features x 16 bytes of pending clouds); the upkeep's scratch is the chain's, sized by the points actually worked
 * on (60 bytes per stored + pending point, 155 232 bytes per segment), not by max_map_points.
 * mml_map_global_download: the LIVE store (xyz: 3 floats per point, cube: its index, cen: 3 ints; any may be NULL). */
int mml_map_global_append(mml_ctx* ctx, int slot, const double* T_wl);
int mml_map_global_increment(mml_ctx* ctx, const double* T_wl, int* n_corner, int* n_surf);
int mml_map_global_download(mml_ctx* ctx, int kind, float* xyz, int* cube, int capacity, int* n, int* cen);
int mml_map_global_reset(mml_ctx* ctx);

/* ---- a12: laserCloud{Corner,Surf}FromMap cube store (Estimator.cpp:1170-1184, Map_Manager.cpp:583-629)
 * The reference hands Estimate() 21*11*21 = 4851 cube clouds plus one kd-tree per cube; processPointToLine /
 * processPointToPlane look the feature's cube up (MAP_MANAGER::FindUsedMap), query THAT cube's tree when the
 * cube holds > 100 corner / > 50 surf points, and fall back to the local map otherwise or when the cube
 * neighbourhood fails the fit.  Here the cubes arrive as ONE concatenated cloud: xyz (3 floats per point) and
 * cube[i] = ToIndex(i, j, k) = i + 21 j + 441 k of point i (points of one cube in the cube cloud's order, so
 * that kd-tree tie order is preserved).  cen: laserCloudCen{Width,Height,Depth}_last (3 ints, NULL keeps
 * the current value, default 10, 5, 10).  m = 0 removes the global map (local-only association).  Every argument -- the
 * kind, m <= max_map_points (MML_ERR_CAPACITY), every cube index in [0, 4851) (MML_ERR_INVALID) -- is checked before anything
 * changes: a refused call leaves the global map as it was. */
int mml_map_set_global(mml_ctx* ctx, int kind, const float* xyz, const int* cube, int m, const int* cen);

/* ---- map banks: N further local maps per context, every scan slot matched against its own ----------------------
 * For several sequences in one context (a fleet's bags, or one bag cut into segments, replayed offline).  A bank is one
 * more local map with the state of the context's own: the 50-entry key-scan ring of corner and surf features with its
 * counts, localMapID, the two kNN grids with their unsorted clouds, the two map sizes.  The context's own map stays as it
 * is; it is what an unbound slot is matched against.  A bank that was never set is an empty map (no feature gets a
 * factor).  Memory per bank: 96 bytes per point of max_map_points, plus 2 x 50 x max_features x 16 bytes from its first
 * increment on.
 * mml_map_banks_create: n_banks in [1, MML_MAP_BANKS_MAX]; a context has one set of banks (MML_ERR_STATE when it has
 * one already).  mml_map_banks_destroy releases them and unbinds every slot; mml_destroy does the same.
 * mml_map_bank_set_local / _reset / _download: mml_map_set_local / mml_map_local_reset / mml_map_local_download on
 * bank `bank`.
 * mml_slot_bind_bank: banks[i] is the bank of slot first_slot + i, -1 the context's own map.  A binding stays until it is
 * changed.  Every call that associates honours it without a further argument: mml_associate, mml_estimate, mml_step (and
 * so the factors mml_fullwindow_solve, mml_fullwindow_solve_batch and mml_fullwindow_marginalize_batch read, which are
 * the ones mml_associate left).  The result of a slot is bit-identical to that of the same call on a context whose own
 * map holds the bank's cloud.  With every slot of a call bound, the context's own map need not be set.
 * CUBE STAGE: a bank has a global cube map of its own -- the MAP_MANAGER store and the copy Estimate() matches against, as
 * the context has them (mml_map_set_global, mml_map_global_*).  A bound slot is matched against its bank's cube first
 * (> 100 corner / > 50 surf points in the feature's cube) and falls back to the bank's local map, exactly as an unbound slot
 * is against the context's own pair; a bank without a cube map is matched against its local map alone.  The context's OWN
 * cube map and bound slots exclude each other: binding a slot to a bank while it is set (mml_map_set_global,
 * mml_map_global_increment) returns MML_ERR_STATE, and so does a call that associates a bound slot after it was set; nothing
 * is changed in either case.
 * mml_map_bank_set_global: mml_map_set_global on bank `bank` (m = 0 removes that bank's cube map).
 * mml_map_bank_global_append: mml_map_global_append for n DISTINCT banks, slot slots[i] at T_wl + 16 i into bank banks[i].
 * mml_map_bank_global_increment: mml_map_global_increment for n DISTINCT banks, bank banks[i] at T_wl + 16 i; n_corner /
 * n_surf: n live store sizes each, or NULL.  The banks are worked through one after the other, each by the chain of
 * mml_map_bank_global_increment_segmented with n = 1 (3 + R host synchronisations per bank, 4 + R when its match copy has
 * to grow); every bank ends bit-identical, the order inside every cube included, to the own cube store of a context with
 * the same history.  A refusal at bank i (its store would exceed max_map_points, its pose needs more than 64 layer shifts)
 * leaves bank i and the banks after it exactly as they were and banks 0 .. i-1 incremented.
 * mml_map_bank_global_download / _reset: mml_map_global_download / _reset on bank `bank` (mml_map_bank_reset keeps its
 * meaning: the local ring only).
 * All five check every argument before the device is touched or anything changes: a NULL context and a bank out of range
 * are MML_ERR_INVALID, a context without banks MML_ERR_STATE, a bank named twice in one append / increment
 * MML_ERR_INVALID; an append of a slot without a down-sampled stack is MML_ERR_STATE for the whole call.
 * Memory per bank for its cube map, from its first append / increment on: 72 bytes per point of max_map_points (the live
 * store and its compaction twin) plus 2 x 16 x max_features x 16 bytes of pending clouds -- 37 748 736 + 4 194 304 bytes at
 * max_map_points = 1 << 19 and max_features = 8192; the match copy is sized by need, 36 bytes per point it holds (at least
 * 1024) plus 16 bytes per point of max_map_points for its cell table, per kind, from the first set_global / increment on.
 * The upkeep's scratch is the context's and is shared by all banks and the own store: the chain's, 60 bytes per point
 * worked on at a time plus 155 232 bytes per segment, grown on demand (a context holds no fixed scratch sized by
 * max_map_points for it).  mml_map_banks_create allocates none of it.
 * mml_slot_bank_get reads the bindings back (all -1 on a context without banks).
 * mml_map_bank_increment: mml_map_increment_local for n DISTINCT banks (a bank named twice is MML_ERR_INVALID, checked
 * with every other argument before anything changes): bank banks[i] takes the stacks of slot slots[i] at T_wl + 16 i.
 * Every bank ends bit-identical to the own map of a context with the same history of increments.  n_corner / n_surf: n
 * new map sizes each, or NULL.  The banks are worked through one after the other, each as mml_map_increment_local works
 * the own map: 2 + R host synchronisations per bank, R the cell-refinement rounds of that bank's slower kind (1 to 5).
 * mml_map_bank_increment_segmented: the same call -- arguments, argument checks, drained context -- with the n banks' work in
 * ONE chain of launches: one launch writes all 2 n stacks into their rings, one concatenates all rings, one stable 64-bit
 * sort keyed (bank of the call, kind) << 32 | voxel filters all of them, and the 2 n kNN grids are built by one sort per
 * cell-refinement round.  Every bank ends bit-identical to what mml_map_bank_increment leaves on the same history: ring,
 * counts, localMapID, the filtered clouds with their order, both grids, the sizes returned.  ONE DIFFERENCE: the stack sizes
 * of all n slots are read in one copy and checked before any bank changes -- a slot without a down-sampled stack is
 * MML_ERR_STATE, the message names the slot, and ALL n banks are exactly as before the call (mml_map_bank_increment leaves
 * banks 0 .. i-1 incremented); a bank whose ring would exceed max_map_points is MML_ERR_CAPACITY in the same way.
 * Host synchronisations after the entry drain: 2 + R whatever n is (the stack sizes; the filtered sizes and boxes; one per
 * cell-refinement round, R = the rounds of the slowest (bank, kind), 1 to 5).  Scratch: 48 bytes per ring point the call
 * works on at a time (both kinds of its banks' rings, the new stacks included) plus the sort's temporary storage, grown on
 * demand and kept until mml_destroy.  A call whose banks hold more than MML_BANK_INCREMENT_BUDGET ring points works them in
 * chunks -- greedy, in call order, a bank over the budget a chunk of its own -- and makes one synchronisation for the stack
 * sizes and 1 + R for every chunk; the default budget keeps every position in an int and the scratch at 192 MiB.
 * mml_debug_bank_increment_budget (a test hook): sets that budget, in points, for the context's later calls.
 * mml_map_bank_global_increment_segmented / mml_map_bank_global_append_segmented: mml_map_bank_global_increment / _append --
 * arguments, argument checks, drained context -- with the n banks' work in ONE chain of launches.  A segment is (bank of the
 * call, kind), 2 n of them behind one device-resident table: one launch tags all rows (a stored point's cube with the MapMove
 * shifts applied as it is read, a pending point's from the moved centre) and fills the per-segment cube histograms, one
 * classifies, ONE scan per flag array runs over all segments, one launch scatters, ONE stable 64-bit sort keyed
 * segment << 53 | cube << 40 | voxel index (over 53 + the bits of the segment count) filters every cube that grew beyond 300
 * points, and the 2 n match copies are built by one sort per cell-refinement round.  This chain is the only implementation:
 * the loop call runs it once per bank with n = 1, mml_map_global_increment / _append once on the own store, and both append
 * entry points are the same call.  Every bank ends bit-identical to what the loop call leaves on the same history -- live
 * store with its tags and the order inside every cube, centre, emptied pending clouds, the match copy (the store at the START
 * of the increment with the centre before MapMove) with its grid and cube counts, the sizes returned.
 * ALL OR NOTHING -- the one difference to the loop increment, which differs only in that its banks 0 .. i-1 stay incremented
 * when bank i is refused.  Every refusal leaves EVERY bank of the call exactly as it was -- live store, tags, centre, pending
 * clouds, match copy -- and n_corner / n_surf unwritten: a bank twice or out of range, n < 1, a context without banks, an
 * append of a slot without a stack (MML_ERR_STATE) or beyond 16 x max_features pending points (MML_ERR_CAPACITY), a store
 * that would exceed max_map_points (MML_ERR_CAPACITY; the message names the bank), a pose that needs more than 64 layer
 * shifts (MML_ERR_INVALID).  The refusals are decided in this order: arguments; poses, on a host copy of every centre; then
 * the one read-back of every segment's kept / selected totals, before which only scratch is
 * written.  The live arrays are read-only until every chunk (below) has passed; the match copies are built after that from
 * the untouched arrays, then the buffer pairs are swapped and the host state is written.
 * Host synchronisations after the entry drain, whatever n is (the loop makes them per bank): 1 for the kept / selected totals
 * of all segments (the capacity decision), 1 for the filtered sizes (none when no cube is filtered), at most 1 when a match copy has to grow, 1
 * for the bounding boxes of all match copies, R for the cell-refinement rounds of the slowest match copy: 3 + R, 4 + R on
 * growth.  The append reads all stack sizes in ONE copy and transforms all 2 n stacks in ONE launch.
 * Scratch: an allocation group of its own, grown on demand and kept until mml_destroy -- 60 bytes per point (store + pending,
 * both kinds) the call works on at a time plus 155 232 bytes (8 x 4851 ints) per segment, and the sorts' temporary storage.
 * A call whose banks hold more than MML_BANK_GLOBAL_INCREMENT_BUDGET points, or more than MML_BANK_GLOBAL_CHUNK_BANKS banks,
 * works them in chunks -- greedy, in call order, a bank over the budget a chunk of its own (as is the one store of a loop or
 * own-store call: the budget hook applies to them and changes nothing) -- with the synchronisations above per chunk; the store chains of ALL chunks run, and pass their capacity decisions, before the first match copy is built.
 * The defaults bound the scratch by 240 MiB + 38 MiB and keep every position in an int.
 * mml_debug_bank_global_increment_budget (a test hook): sets that budget, in points, for the context's later calls. */
#define MML_MAP_BANKS_MAX 1024
#define MML_BANK_INCREMENT_BUDGET (1 << 22)
#define MML_BANK_GLOBAL_INCREMENT_BUDGET (1 << 22)
#define MML_BANK_GLOBAL_CHUNK_BANKS 128
int mml_map_banks_create(mml_ctx* ctx, int n_banks);
int mml_map_banks_destroy(mml_ctx* ctx);
int mml_map_bank_set_local(mml_ctx* ctx, int bank, int kind, const float* xyz, int m);
int mml_map_bank_reset(mml_ctx* ctx, int bank);
int mml_map_bank_download(mml_ctx* ctx, int bank, int kind, float* xyz, int capacity, int* n);
int mml_slot_bind_bank(mml_ctx* ctx, int first_slot, int count, const int* banks);
int mml_slot_bank_get(mml_ctx* ctx, int first_slot, int count, int* banks);
int mml_map_bank_increment(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl, int* n_corner, int* n_surf);
int mml_map_bank_increment_segmented(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl, int* n_corner, int* n_surf);
int mml_debug_bank_increment_budget(mml_ctx* ctx, long points);
int mml_map_bank_set_global(mml_ctx* ctx, int bank, int kind, const float* xyz, const int* cube, int m, const int* cen);
int mml_map_bank_global_append(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl);
int mml_map_bank_global_increment(mml_ctx* ctx, int n, const int* banks, const double* T_wl, int* n_corner, int* n_surf);
int mml_map_bank_global_increment_segmented(mml_ctx* ctx, int n, const int* banks, const double* T_wl, int* n_corner, int* n_surf);
int mml_map_bank_global_append_segmented(mml_ctx* ctx, int n, const int* banks, const int* slots, const double* T_wl);
int mml_debug_bank_global_increment_budget(mml_ctx* ctx, long points);
int mml_map_bank_global_download(mml_ctx* ctx, int bank, int kind, float* xyz, int* cube, int capacity, int* n, int* cen);
int mml_map_bank_global_reset(mml_ctx* ctx, int bank);

/* Exact 5-NN against a local map (twin of kdtree->nearestKSearch(p, 5, idx, d2), Estimator.cpp:284,704):
 * q: nq x 3 host floats (already in the map frame); idx: nq x 5 (indices into the uploaded cloud,
 * ascending d2, ties by lower index), d2: nq x 5 (float, ((dx*dx+dy*dy)+dz*dz)). max_d2: search bound
 * (neighbours are exact for every query whose 5th distance is < max_d2; others report -1 / inf). */
int mml_knn5(mml_ctx* ctx, int kind, const float* q, int nq, float max_d2, int* idx, float* d2);

/* ---- a11..a16: association + model fit -------------------------------------------------------------
 * Estimator::processPointToLine (Estimator.cpp:148-365) and processPointToPlanVec (:573-777) on the
 * local maps for `count` slots.  T_wl: count x 16 (transformTobeMapped, :1268-1270).  Factors stay on
 * the device.  stats (count entries) may be NULL: the call then only enqueues (T_wl is staged before it returns, nothing
 * is read back, no synchronisation) -- what a caller does that goes straight on to mml_solve on the same slots. */
typedef struct {
    int n_line, n_plane;        /* factors produced (vLineFeatures / vPlanFeatures sizes) */
    int n_line_used, n_plane_used; /* with |error| > 1e-5 (Estimator.cpp:1385,1396) */
    double normal_gram[9];      /* sum of omega omega^T over plane factors */
    double min_singular;        /* checkLocalizability (:536-565): sqrt(lambda_min(gram)), -1 if n_plane <= 10 */
    int is_degenerate;          /* min_singular < 3.0 (:772-775) */
} mml_assoc_stats;
int mml_associate(mml_ctx* ctx, int first_slot, int count, const double* T_wl, double thres_dist,
                  mml_assoc_stats* stats /* count entries, may be NULL */);

/* Factor read-back for parity tests.  line: n x 10 doubles (pointOri, P1, P2, error) plus src feature
 * index; plane: n x 10 doubles (pointOri, pointProj, omega, error). Capacity in factors. */
int mml_factors_download(mml_ctx* ctx, int slot, int kind, double* out, int* src, int capacity, int* n);
/* The inverse: n factor records in the layout of mml_factors_download become the slot's vLineFeatures (kind 0) /
 * vPlanFeatures (kind 1) -- for callers that keep FeatureLine / FeaturePlanVec objects of their own (the outputs of
 * Estimator::processPointToLine / processPointToPlanVec, Estimator.h:159-186) and only want the solve, and for the
 * known-answer tests of the residual functors (a factor whose point lies exactly on its line).  Record i gets src = i and
 * the slot's feature count of that kind becomes n (the down-sampled stack no longer corresponds to the factors);
 * point / line end points / omega are stored as floats, as the reference's members are (Estimator.cpp:256-271,643-653). */
int mml_factors_upload(mml_ctx* ctx, int slot, int kind, const double* rec, int n);

/* ---- a17..a20: residual + Jacobian + normal equations ------------------------------------------------
 * Cost_NavState_IMU_Line / Cost_NavState_IMU_Plan_Vec (include/utils/ceresfunc.h:397-458, 517-570) with
 * analytic Jacobians, Ceres' Huber correction and the J^T J / J^T r reduction for one slot at pose
 * x = [t, phi].  T_bl: 16 doubles.  H: 36, g: 6, cost: 1 (host). */
int mml_linearize(mml_ctx* ctx, int slot, const double* x, const double* T_bl, double plan_weight_tan,
                  double huber_delta, double* H, double* g, double* cost);

/* The same for the `frames` (<= 8) consecutive slots of a window in ONE launch and one read-back: frame f is linearised
 * at x + f * x_stride (6 doubles [t, phi]; x_stride = 15 walks the [PR | VBias] states of the full-window solver) and
 * its record (MML_NEQ_RECORD_DOUBLES doubles, layout below) is written to records + 32 f.  This is what one trust-region
 * evaluation of Estimator::Estimate costs on the device side (Estimator.cpp:1265-1299 loops over the frames). */
int mml_linearize_window(mml_ctx* ctx, int first_slot, int frames, int x_stride, const double* x, const double* T_bl,
                         double plan_weight_tan, double huber_delta, double* records);

typedef struct {
    int max_num_iterations;  /* Estimator.cpp:1428 (10) */
    int fixed_iterations;    /* != 0: run exactly max_num_iterations, no convergence tests */
    double huber_delta;      /* 0.1 / lidar_m in 1-frame mode (:1216-1222); <= 0: no loss */
    double plan_weight_tan;  /* :1203 / :1206 */
} mml_solve_opts;
typedef struct {
    int iterations, successful;
    double initial_cost, final_cost;
    int termination;         /* 0 max iterations, 1 gradient, 2 parameter, 3 function tolerance, 4 failure (5 consecutive
                                invalid steps: the poses are handed back as they came in, as Solver::Solve does) */
} mml_solve_summary;
/* ceres::Solve replacement (Estimator.cpp:1425-1432): trust-region dogleg on the device, one problem per
 * window of `window` consecutive slots (window = 1: the reference's live 1-frame mode).  x: count x 6
 * in/out; summaries: count / window entries (may be NULL); trace (may be NULL): per problem
 * max_num_iterations x (6*window) doubles, x after every iteration (rows past summaries[p].iterations repeat the
 * final x). */
int mml_solve(mml_ctx* ctx, int first_slot, int count, int window, const double* T_bl,
              const mml_solve_opts* opts, double* x, mml_solve_summary* summaries, double* trace);

/* ---- a21: Estimator::Estimate, 1-frame mode (Estimator.cpp:1143-1581) -------------------------------
 * Outer loop (re-associate with thres_dist 25 -> 10 -> 1, solve, convergence test) for `count` slots.
 * P: count x 3, Q: count x 4 (body pose in/out), exTlb: 16.  Requires mml_downsample first. */
typedef struct {
    int outer_iterations;
    int is_degenerate;
    int n_corner_feat, n_surf_feat;
} mml_estimate_info;
int mml_estimate(mml_ctx* ctx, int first_slot, int count, const double* exTlb, double* P, double* Q,
                 int max_outer, int inner_iters, mml_estimate_info* info /* count entries or NULL */);

/* ---- localisation in a surfel world map ("The world map", "Surfel maps" above) ----------------------------------------------
 * mml_world_map_export / _import: a map leaves the device and comes back bit for bit.  Export runs the collect / sort / gather
 * chain of the downloads with a raw gather: row r is the voxel of row r of the other downloads; ijk = the voxel indices of its
 * key (i, j, k), sums = the stored float4 (NOT the centroid), counts = the point counts, moments = the stored 12 floats (a surfel
 * map; must be NULL on a plain one).  ijk, sums and counts all NULL: the sizing call.  MML_ERR_CAPACITY when `capacity` (voxels)
 * is below the count.  Import inserts n voxels into `map`, one lane per voxel, plain stores; a later mml_world_map_add goes on
 * from the stored sums.  Checked on the host before any device work, each MML_ERR_INVALID: an index outside [-2^17, 2^17) or the
 * voxel whose packed key is the free marker (map 1023, all three indices 2^17 - 1), counts[r] < 1, a duplicate row, moments NULL
 * on a surfel map or non-NULL on a plain one, a NULL array with n > 0, n < 0.  Then, as mml_world_map_add, one lookup launch and
 * ONE read-back: MML_ERR_STATE if a voxel of the call is present already, MML_ERR_CAPACITY naming the figures if the voxels held
 * plus n exceed capacity_voxels; either way the table is bit for bit what it was.  The call returns with the rows stored.
 *
 * mml_world_map_associate: plane factors for the surf stack (kind 1, as mml_downsample left it) of slot first_slot + i from the
 * surfels of map map_of_slot[i] (-1: the slot is skipped and left as it is), count slots in ONE launch.  The arithmetic is
 * csrc/world_map_assoc.h (host and device), per feature f of index s:
 *   w           the float world point of f at the slot's pose (the function mml_world_map_add uses); f is skipped when a
 *               coordinate of w is not finite or a voxel index of w leaves [-2^17, 2^17);
 *   candidates  the voxel (i, j, k) of w (neighbourhood 0) or the 27 voxels (i + di, j + dj, k + dk), di dj dk in {-1, 0, 1},
 *               that lie in range, each looked up read-only under the slot's map and kept when its count >= min_points; c =
 *               sum.xyz / (float)count in float; r2 = ((wx-cx)^2 + (wy-cy)^2) + (wz-cz)^2, differences and products in double;
 *               the smallest r2 wins, ties go to the smaller packed key; no candidate: no factor;
 *   gates       the winner's surfel record (the function mml_world_map_download_surfels runs) -- planarity < min_planarity: no
 *               factor, and no second choice; d = (nx*(wx-cx) + ny*(wy-cy)) + nz*(wz-cz) in double; |d| > max_plane_dist: none;
 *   record      ori = f, omega = (nx, ny, nz) as stored, proj_a = (double)w_a - d * (double)n_a, error = |T f - proj| as
 *               mml_associate computes a plane factor's, src = s.
 * The slot is left as mml_associate leaves it: plane records at index s of the slot's list (none: src = -1), NO line factors,
 * the statistics as mml_associate produces them; mml_linearize*, mml_solve and mml_factors_download work on it unchanged.
 * Host synchronisations: ONE, the read-back of the slots' stack sizes that the refusal below needs, and one more when stats is
 * given; with stats NULL the launch itself is only enqueued behind that read-back.  The table is only read.  Refused before anything is written, the message names the slot:
 * MML_ERR_STATE without a world map, on a plain map, or for a slot that takes part and holds no down-sampled stack;
 * MML_ERR_INVALID for a slot range outside the context, count outside 1 .. 65535, a map outside [-1, n_maps), min_points < 3,
 * neighbourhood other than 0 / 1, a non-finite or negative gate, NULL map_of_slot / T_wl / opts.
 *
 * mml_world_map_localize: mml_estimate's outer loop and convergence test with mml_world_map_associate in the place of
 * mml_associate and max_plane_dist_by_outer[min(outer, 2)] in the place of the 25 -> 10 -> 1 schedule (opts->assoc.max_plane_dist
 * itself is not read); the solve and its options are mml_estimate's.  Every slot of the call must name a map (no -1).  One host
 * synchronisation per outer iteration, as mml_estimate, and one more at entry (the stack sizes).  The maps are only read. */
typedef struct {
    int   neighbourhood;      /* 0: the point's own voxel, 1: the 27 voxels around it (default 1) */
    int   min_points;         /* a voxel takes part from this count on; >= 3 (default 5) */
    float min_planarity;      /* gate on the surfel's planarity (default 0.5) */
    double max_plane_dist;    /* gate on |d|, metres */
} mml_wm_assoc_opts;
typedef struct {
    mml_wm_assoc_opts assoc;
    double max_plane_dist_by_outer[3];
    int max_outer, inner_iters;
} mml_wm_localize_opts;
void mml_wm_assoc_opts_default(mml_wm_assoc_opts* opts, float leaf);   /* max_plane_dist = leaf */
void mml_wm_localize_opts_default(mml_wm_localize_opts* opts, float leaf);  /* 2 leaf, leaf, leaf / 2; 5 outer, 10 inner */
int mml_world_map_export(mml_ctx* ctx, int map, int* ijk /* n x 3 */, float* sums /* n x 4 */, int* counts,
                         float* moments /* n x 12, NULL on a plain map */, long capacity, long* n_voxels);
int mml_world_map_import(mml_ctx* ctx, int map, long n, const int* ijk, const float* sums, const int* counts,
                         const float* moments);
int mml_world_map_associate(mml_ctx* ctx, int first_slot, int count, const int* map_of_slot /* -1 skips */,
                            const double* T_wl /* count x 16 */, const mml_wm_assoc_opts* opts,
                            mml_assoc_stats* stats /* count entries or NULL: nothing is read back behind the launch */);
int mml_world_map_localize(mml_ctx* ctx, int first_slot, int count, const int* map_of_slot, const double* exTlb,
                           double* P, double* Q, const mml_wm_localize_opts* opts, mml_estimate_info* info);

/* ---- relocalisation in a surfel world map: pose hypotheses scored on the device, a coarse-to-fine search -------------------
 * mml_world_map_score: how well the surf stack of slot first_slot + i fits map map_of_slot[i] at each of n_hyp pose hypotheses
 * (T_wl: count x n_hyp x 16, row-major lidar poses as mml_world_map_associate takes them), count x n_hyp results from ONE launch.
 * The arithmetic is csrc/world_map_score.h (host and device).  Of the stack the call looks at the features 0, stride, 2 stride,
 * ...; each goes through exactly the steps of mml_world_map_associate above: the world point; skipped when it has no voxel; the
 * candidates and the choice; the winner's surfel normal and planarity; the two gates.  A feature that mml_world_map_associate
 * would make a factor of is a match and contributes
 *     q = (unsigned)((1.0 - fabs(d) / max_plane_dist) * 65536.0)     double arithmetic, truncated: 0 .. 65536
 * with d the plane distance of the gate (a d that is not a number contributes 0).  Per (slot, hypothesis): n_scored = the features
 * looked at and not skipped, n_match = the matches, score_q = the sum of q.  All three are integers: a result does not depend on
 * summation order, launch geometry or batching, and is compared exactly.  A hypothesis with an entry that is not finite is not
 * refused: its features have no voxel, n_scored = 0.  A slot with map -1 is skipped: its rows are zeros.
 * Ranking, wherever a best hypothesis is chosen: the larger score_q, then the larger n_match, then the smaller index.
 * The surfel cache: the first call that scores allocates one float4 (nx, ny, nz, planarity) per table position in the map's
 * memory, 16 bytes per position more (MML_ERR_HIP before any launch if that fails), filled by one kernel, one lane per position,
 * with the function mml_world_map_download_surfels runs.  mml_world_map_add (past its refusal point), _import, _reset, _create*
 * and _destroy mark it stale on the host; the next score call rebuilds it first.  A match then costs one 16-byte load where the
 * association loads 36 bytes of moments and runs the eigen-solver.  mml_world_map_associate itself does not use the cache.
 * Host synchronisations: the read-back of the stack sizes at entry (the refusal of a slot without a stack, as in
 * mml_world_map_associate) and ONE more, the read-back of the results.  The table, the slots, their factors and statistics are
 * only read.  Refused before anything is written, the message names the offender: everything mml_world_map_associate refuses;
 * MML_ERR_INVALID for n_hyp outside 1 .. 65536, count * n_hyp above 2^22, stride < 1, max_plane_dist not finite or <= 0 (the
 * quantisation divides by it), NULL T_wl / out.
 *
 * mml_wm_pose_grid (host, no context): the hypotheses of a grid around the pose seed_T16.  Cells per axis: 2 floor(half / step) +
 * 1 (the quotient is taken with 1e-9 added, so that 0.6 / 0.2 counts three steps); half = 0: one cell, the step is not read.  x
 * and y share half_xy / step_xy.  Index ((iyaw nz + iz) ny + iy) nx + ix; cell c of an axis is offset (c - floor(half / step))
 * step.  Hypothesis = Trans(t_seed + (dx, dy, dz)) Rz(yaw) R_seed: a shift along the world axes and a turn about the world z axis
 * through the lidar's origin.  When the yaw cells cover the whole circle (2 floor(half_yaw / step_yaw) step_yaw = 2 pi to 1e-9)
 * the last one, which would repeat the first, is dropped.  out NULL: the sizing call, *n_hyp alone.  MML_ERR_INVALID for an
 * argument that is not finite, a negative half, half_yaw > pi, a step <= 0 on an axis with half > 0, NULL seed / n_hyp, more than
 * 2^22 cells; MML_ERR_CAPACITY when capacity (hypotheses) is below the count (*n_hyp is set).
 * mml_wm_body_pose (host): P, Q of the body from a lidar pose T_wl and exTlb -- the inverse of the composition mml_estimate and
 * mml_world_map_localize apply to P, Q (T_wl = [Q, P] inverse(exTlb)); the conversion mml_world_map_relocalize hands T_start to
 * its loop with.  mml_wm_lidar_pose (host): that composition itself, T_wl from P, Q and exTlb -- the seed of the level-0 grid and
 * the pose `final` is scored at.
 *
 * mml_world_map_relocalize: a coarse-to-fine search around the seed poses P, Q of `count` slots, ending in
 * mml_world_map_localize.  Level 0 scores mml_wm_pose_grid around every slot's seed lidar pose in one mml_world_map_score; the
 * `keep` best hypotheses per slot (all of them when the grid has fewer) are chosen on the host; each further level divides every
 * step by `refine` and scores, again in one call for all slots, the grids of +-1 previous step around the kept hypotheses in
 * their order (index = kept rank x cells + cell).  The best hypothesis of the last level is T_start; one
 * mml_world_map_localize runs over the count slots from mml_wm_body_pose(T_start); one last score call at the result fills
 * `final`.  info[i]: best = the score of the best level-0 hypothesis; second = that of the best level-0 hypothesis that is not
 * its neighbour (index distance > 1 on some axis, yaw cyclic when the grid covers the circle; zeros when there is none) -- its
 * ratio to best is the caller's ambiguity measure, the call applies no threshold; n_hyp_scored = the hypotheses of all levels;
 * est = mml_world_map_localize's.  All slots share one grid shape.  Host synchronisations: one at entry (the stack sizes), one per
 * level, mml_world_map_localize's (one at entry and one per outer iteration) and one for `final`.  Refused before anything is
 * written: what the score and the loop refuse, levels outside 1 .. 3, refine outside 2 .. 4, keep outside 1 .. 16, what
 * mml_wm_pose_grid refuses, a level of more than 65536 hypotheses per slot or 2^22 per call. */
typedef struct { unsigned long long score_q; int n_match; int n_scored; } mml_wm_score;
typedef struct { mml_wm_assoc_opts assoc; int stride; } mml_wm_score_opts;  /* features 0, stride, 2 stride, ...; stride >= 1 */
void mml_wm_score_opts_default(mml_wm_score_opts* opts, float leaf);         /* assoc defaults, max_plane_dist = leaf, stride 1 */
int mml_world_map_score(mml_ctx* ctx, int first_slot, int count, const int* map_of_slot /* -1 skips: its results are zeros */,
                        int n_hyp /* per slot, 1..65536; count * n_hyp <= 2^22 */, const double* T_wl /* count x n_hyp x 16 */,
                        const mml_wm_score_opts* opts, mml_wm_score* out /* count x n_hyp */);
typedef struct {
    double half_xy, step_xy, half_z, step_z;   /* metres, world axes; half 0: one cell on that axis */
    double half_yaw, step_yaw;                 /* radians about the world z axis through the lidar's origin; half_yaw <= pi */
    int levels;                                /* 1..3 */
    int refine;                                /* 2..4: a further level divides every step by this and spans +-1 previous step */
    int keep;                                  /* 1..16 hypotheses carried from one level to the next */
    mml_wm_score_opts score;
    mml_wm_localize_opts localize;
} mml_wm_reloc_opts;
typedef struct { mml_wm_score best, second, final; long n_hyp_scored; double T_start[16]; mml_estimate_info est; } mml_wm_reloc_info;
/* 2 m / 0.5 m in x and y, one z cell, the whole circle in steps of pi / 16; 2 levels, refine 2, keep 4; the score's and the
 * loop's defaults for the leaf */
void mml_wm_reloc_opts_default(mml_wm_reloc_opts* opts, float leaf);
int mml_wm_pose_grid(const double* seed_T16, double half_xy, double step_xy, double half_z, double step_z, double half_yaw,
                     double step_yaw, double* out /* H x 16 or NULL: sizing */, long capacity, long* n_hyp);
int mml_wm_body_pose(const double* T_wl, const double* exTlb, double* P /* 3 */, double* Q /* 4: x y z w */);
int mml_wm_lidar_pose(const double* P, const double* Q, const double* exTlb, double* T_wl /* 16 */);
int mml_world_map_relocalize(mml_ctx* ctx, int first_slot, int count, const int* map_of_slot, const double* exTlb,
                             double* P, double* Q /* in: seed body poses; out: result */, const mml_wm_reloc_opts* opts,
                             mml_wm_reloc_info* info /* count entries or NULL */);

/* ---- eviction: voxels leave the world map by box and by count, their rows handed back --------------------------------------
 * mml_world_map_evict: one rule per map named, n_rules maps in ONE device chain; the decision per voxel is
 * csrc/world_map_evict.h's mml_wme_goes (host and device, integers only): the box test by mode -- OUTSIDE: a voxel goes unless
 * lo[a] <= index[a] < hi[a] on all three axes, INSIDE: it goes if so, NOBOX: the box is not read -- OR count < min_count.  A box
 * with lo[a] >= hi[a] on some axis is empty: OUTSIDE then empties the map, INSIDE evicts nothing by the box.
 *   maps not named     keep every bit of theirs.
 *   survivors          keep sum, count and moments bit for bit; which table position holds them may change, and nothing a call
 *                      returns depends on that.  Every survivor is found by every later call (add, import, associate, score); an
 *                      evicted voxel is not, and an add into its place starts from zero: the table is rebuilt (the survivors of
 *                      ALL maps taken out, the keys cleared, the survivors put back by claim, as mml_world_map_reset does for one
 *                      map), no free marker is stored into a probe chain.
 *   rows               the evicted voxels in ascending packed-key order -- map, then k, j, i --, so one map's rows are one run in
 *                      the order of mml_world_map_export, beginning at info[r].first_row, in the layout mml_world_map_import
 *                      takes (ijk, stored sums, counts, the 12 stored moments on a surfel map); out_map[row] = the map.  Evicting a
 *                      voxel and importing its row leaves every export what it was, bit for bit.  out_map, out_ijk, out_sums,
 *                      out_counts and out_moments all NULL with capacity 0: the voxels are dropped, nothing is handed back.
 *   counts, version    mml_world_map_size is right afterwards; the surfel cache is marked stale exactly when the table is
 *                      written: not by a dry run, not by a call that evicts nothing (the table is untouched), not by a refusal.
 *   MML_WM_EVICT_DRY   counts only (info, *n_evicted): nothing but scratch is written, out arrays and capacity are not used.
 * Host synchronisations: ONE, the read-back of the counters behind the marking pass -- the refusal point: MML_ERR_CAPACITY naming
 * both figures when rows are wanted and capacity < the voxels to evict, info and *n_evicted filled, the table bit for bit what it
 * was -- and a second one only when rows are handed back (the copies up).  The rebuild costs a pass over the whole table however
 * few voxels go.  Scratch per voxel of capacity_voxels: 12 bytes for a dry run, 32 (80 on a surfel map) when the rows are dropped,
 * 44 (92) when they are handed back, grow-only, MML_ERR_HIP before any launch when it cannot grow.
 * Refused before anything is written, the message names the rule: MML_ERR_STATE without a world map; MML_ERR_INVALID for NULL
 * rules, n_rules outside 1 .. n_maps, a map outside [0, n_maps), a map named twice, an unknown mode, min_count < 0, unknown flag
 * bits, capacity < 0, out arrays partly NULL (or a capacity without them), out_moments given on a plain map or missing on a
 * surfel map when rows are wanted.
 * mml_wm_index_box (host, no context): the index box of a metric one with mml_world_map_add's arithmetic (inv = 1.0f / leaf, the
 * product in float, floor): lo = index(lo_xyz), hi = index(hi_xyz) + 1, each clamped to [-2^17, 2^17].  MML_ERR_INVALID for a
 * coordinate or a leaf that is not finite, a leaf <= 0, a NULL array. */
#ifndef MML_WM_EVICT_RULE_DEFINED
#define MML_WM_EVICT_RULE_DEFINED
#define MML_WM_EVICT_OUTSIDE 0   /* voxels outside the box go */
#define MML_WM_EVICT_INSIDE  1   /* voxels inside the box go  */
#define MML_WM_EVICT_NOBOX   2   /* the box is not read; only min_count decides */
typedef struct {
    int map;            /* 0 .. n_maps-1; a map may be named by at most one rule of a call */
    int mode;
    int lo[3], hi[3];   /* voxel indices i, j, k: inside means lo[a] <= index[a] < hi[a] on all three axes */
    int min_count;      /* a voxel whose point count is < min_count goes as well; 0 or 1: none does */
} mml_wm_evict_rule;
#endif
typedef struct { long n_before, n_evicted, n_kept, first_row; } mml_wm_evict_info;   /* per rule */
#define MML_WM_EVICT_DRY 1u      /* count only: nothing is written anywhere on the device but scratch */
int mml_wm_index_box(float leaf, const float lo_xyz[3], const float hi_xyz[3], int lo[3], int hi[3]);
int mml_world_map_evict(mml_ctx* ctx, int n_rules, const mml_wm_evict_rule* rules, unsigned flags,
                        mml_wm_evict_info* info /* n_rules, may be NULL */, long capacity /* rows the out arrays hold */,
                        int* out_map, int* out_ijk /* n x 3 */, float* out_sums /* n x 4 */, int* out_counts,
                        float* out_moments /* n x 12; NULL on a plain map */, long* n_evicted /* may be NULL */);

/* ---- the benchmarked step ---------------------------------------------------------------------------
 * One pass of the hot path over slots [first, first+count) with inputs already uploaded:
 * extract -> undistort -> downsample -> associate (1 pass, thres_dist) -> `gn_iters` trust-region
 * iterations (fixed count).  Everything stays on the device; poses: count x 6 ([t,phi], device-updated,
 * copied back).  This is what bench.py times.  The batch is spread over the context's stream lanes (mml_set_lanes), every
 * lane ordered behind whatever the context's stream holds when the call is made (no synchronisation is needed between
 * mml_scan_upload and mml_step); inside a lane the stages run in order on the lane's stream; the call returns with every
 * stream of the context drained.  The association statistics of mml_associate (counts, normal Gram matrix) are not part of
 * the step; an entry point that needs them afterwards (mml_linearize*, mml_associate with `stats`) computes them on demand.
 * Of the cloud the step itself undistorts the labelled points only -- all its down-sampler reads; the undistortion of the full
 * cloud is completed by the first entry point that reads the slot's cloud afterwards (mml_scan_download*,
 * mml_cloud_download_registered*, mml_slot_digest, mml_undistort, mml_downsample, mml_gicp_refresh*), which then returns what it
 * returned when the step did all of it; a caller that takes poses and feature stacks only never pays for that pass.
 * ($MML_LAZY_UNDISTORT=0, read when the context is created: the step undistorts the whole cloud itself.) */
int mml_step(mml_ctx* ctx, int first_slot, int count, const double* dR, const double* dt,
             const double* exTlb, double thres_dist, int gn_iters, double* x_inout);

/* ---- multi-GPU window solve (one frame per GPU) ---------------------------------------
 * Record layout of one frame's normal equations for the all-gather: 32 doubles =
 * [H upper triangle row-major (21), g (6), cost (1), n_line_used, n_plane_used, 0, 0]. */
#define MML_NEQ_RECORD_DOUBLES 32
/* Writes the record of `slot` at pose x to a DEVICE buffer (32 doubles) -- e.g. a torch tensor's
 * data_ptr() that is then passed to all_gather. Stream-ordered; call mml_synchronize before the collective. */
int mml_linearize_record(mml_ctx* ctx, int slot, const double* x, const double* T_bl, double plan_weight_tan,
                         double huber_delta, double* d_record);
/* Host-side joint dogleg state machine over W gathered records (pure host code, no device needed):
 * restates the same trust-region iteration as mml_solve for a block-diagonal window. */
typedef struct mml_window_solver mml_window_solver;
mml_window_solver* mml_window_solver_create(int W, const mml_solve_opts* opts);
void mml_window_solver_destroy(mml_window_solver* s);
/* Feed the records evaluated at the point last returned in x_eval (first call: the initial x).  On return
 * x_eval holds the next point to linearise at; returns 1 when finished (x_eval = solution), 0 to continue,
 * < 0 on error. */
int mml_window_solver_step(mml_window_solver* s, const double* records /* W x 32 */, double* x_eval /* W x 6 */);
int mml_window_solver_summary(const mml_window_solver* s, mml_solve_summary* out);

/* ---- multi-GPU: RCCL inside the C-ABI ---------------------------------------------------------------
 * One process per GPU, one ctx per process.  The caller distributes the 128-byte id of rank 0 by whatever means it
 * has (a ROS parameter, a file, torch.distributed, MPI); mml_comm_init is collective (ncclCommInitRank on the ctx
 * device).  Collectives run on the ctx stream over RCCL / xGMI; no host round trip inside them. */
#define MML_COMM_ID_BYTES 128
int mml_comm_unique_id(uint8_t* id /* MML_COMM_ID_BYTES, filled by the calling rank */);
int mml_comm_init(mml_ctx* ctx, int n_ranks, int rank, const uint8_t* id);
int mml_comm_destroy(mml_ctx* ctx);   /* also done by mml_destroy */
int mml_comm_info(mml_ctx* ctx, int* n_ranks, int* rank);
/* ncclGetVersion of the RCCL copy the entry points of this section are bound to (MAJOR * 10000 + MINOR * 100 + PATCH). */
int mml_rccl_version(int* version);
typedef struct {
    int evaluations;     /* linearisations of the own frames that did work */
    int rounds;          /* kernels enqueued (max_num_iterations + 2) */
    int exchanges;       /* all-gathers enqueued */
    double device_ms;    /* HIP events on the ctx stream around the whole solve */
} mml_window_timing;
/* The joint window solve of Estimator::Estimate across ranks (Estimator.cpp:1265-1299 evaluates the frames of the
 * window one after the other, :1425-1432 solves): the window holds W = n_ranks * n_local frames (<= 8), rank r owns
 * frames [r * n_local, (r + 1) * n_local) in its slots [first_slot, first_slot + n_local), already associated
 * (mml_associate).  Per trust-region evaluation every rank linearises its own frames on the device, the
 * MML_NEQ_RECORD_DOUBLES-double records travel by ncclAllGather, and every rank advances the same device-resident
 * dogleg state machine (the iteration of mml_solve), so all ranks finish with bit-identical poses and no second
 * broadcast.  x_local: n_local x 6 in/out (own frames); x_window (may be NULL): W x 6 out; summary / timing may be
 * NULL.  Collective: every rank of the communicator must call it with the same n_local and opts. */
int mml_window_solve_allgather(mml_ctx* ctx, int first_slot, int n_local, const double* T_bl, const mml_solve_opts* opts,
                               double* x_local, double* x_window, mml_solve_summary* summary, mml_window_timing* timing);
/* Map-update exchange: the down-sampled corner / surf stacks of `slot` on rank `root` replace those of `slot` on
 * every rank (ncclBroadcast, stream-ordered), so that each replica can run the same mml_map_increment_local /
 * mml_map_global_append (the key-scan update of Estimator.cpp:1083-1085, 1125-1130).  Collective. */
int mml_comm_broadcast_features(mml_ctx* ctx, int slot, int root);
/* Replicates rank `root`'s local maps (both kinds, as set or as grown on the device) on every rank and builds the
 * kNN grids there.  Collective; synchronises the ctx. */
int mml_comm_broadcast_local_map(mml_ctx* ctx, int root);

/* ---- loopback group: the N-rank path on ONE device (test / bring-up entry points) -------------------------------------
 * RCCL refuses two ranks on one device, so the rank > 0 side of the three exchanges above -- the section offsets of the
 * gather buffers, "linearise only my frames", a broadcast whose root is another rank -- cannot run through mml_comm_init on
 * a single-GPU box.  A loopback group makes n_ranks contexts of ONE process on ONE device the ranks 0 .. n_ranks-1
 * (ctxs[r] = rank r) of a communicator whose collectives are executed by the calling thread as device-to-device copies
 * between the ranks' buffers; kernels, buffers and the device-resident state machine are those of the RCCL path.  Each
 * call drives ALL ranks (it is the collective).  Not a deployment mode: no overlap, every exchange drains the streams. */
int mml_comm_init_loopback(mml_ctx** ctxs, int n_ranks);
/* mml_window_solve_allgather for every rank of the group: rank r owns window frames [r * n_local, (r + 1) * n_local) in
 * its slots [first_slot[r], first_slot[r] + n_local).  x_window_in: W x 6 starting poses; x_window_out: n_ranks x W x 6,
 * the window as EVERY rank ends up holding it (they must be identical); summaries (may be NULL): n_ranks. */
int mml_window_solve_allgather_loopback(mml_ctx** ctxs, int n_ranks, const int* first_slot, int n_local, const double* T_bl,
                                        const mml_solve_opts* opts, const double* x_window_in, double* x_window_out,
                                        mml_solve_summary* summaries);
int mml_comm_broadcast_features_loopback(mml_ctx** ctxs, int n_ranks, int slot, int root);
int mml_comm_broadcast_local_map_loopback(mml_ctx** ctxs, int n_ranks, int root);

/* ---- verification hook: digests of the per-slot state -------------------------------------------------------------------
 * One 64-bit digest per slot for each piece of state the path leaves behind, computed on the device from what the download
 * entry points would hand out (so a digest can be recomputed on the host from mml_scan_download / mml_features_download /
 * mml_factors_download output: tests/conftest.py host_digest), for checks over batches too large to download slot by slot --
 * e.g. "every slot that was given the same scan holds the same result" at the benchmark's launch shapes.  Every word is a
 * sum over the elements e of the piece of  mix(mix(index(e)) ^ field bits ...)  (splitmix64 finaliser), i.e. independent of
 * the order the elements are stored or visited in.  out: count x MML_DIGEST_WORDS.  Pieces (what they are in the reference):
 *   0 counts       n_points, n_velo, the four union_cloud.msg *_num (union_cloud.msg:4-19), both stack sizes
 *   1 label        normal_z of every fused point, keyed by its index in [velo_combine ; livox_combine]
 *                  (unionFeatureExtract.cpp:1016-1032,1233-1252)
 *   2 line         normal_y (ring / Livox line, :1186, :997)
 *   3 xyzi         x, y, z, intensity -- after mml_undistort the output of RemoveLidarDistortion (unionPoseEstimation.cpp:402-421)
 *   4 reltime      normal_x
 *   5 / 6          corner / surf stack after pcl::VoxelGrid (Estimator.cpp:1015-1024), keyed by position in the stack
 *   7 / 8          line / plane factor records as mml_factors_download returns them (Estimator.h:59-122), keyed by src
 *   9 pose         the 6 doubles of the slot's pose after the last solve (Estimator.cpp:937-964 para_PR)
 * Synchronous. */
#define MML_DIGEST_WORDS 10
int mml_slot_digest(mml_ctx* ctx, int first_slot, int count, uint64_t* out);

/* ---- measurement hooks ----------------------------------------------------------------------------------
 * With profiling on, every kernel launch is bracketed by HIP events on the ctx stream. */
#define MML_MAX_STAGES 32
typedef struct {
    int n_stages;
    const char* name[MML_MAX_STAGES];
    double total_ms[MML_MAX_STAGES];
    long launches[MML_MAX_STAGES];
} mml_profile;
/* ---- IMU factor, marginalization prior, full-window solve (host side) --------------
 * O(W) dense work on <= 8 frames x 15 parameters; the per-frame lidar normal equations come from the device
 * (mml_linearize_record / the all-gather of section 8(e)).  No device is needed for these entry points. */
typedef struct {
    double dp[3], dv[3];
    double dq[4];             /* x, y, z, w */
    double dtime;
    double bg[3], ba[3];      /* linearized_bg / linearized_ba */
    double jacobian[225];     /* 15 x 15 row-major, order P R V BG BA (IMUIntegrator.h:86-93) */
    double covariance[225];
} mml_imu_preint;
/* IMUIntegrator::PreIntegration (IMUIntegrator.cpp:108-166).  samples: n x 7 doubles = angular_velocity xyz,
 * linear_acceleration xyz as in the message (multiplied by gnorm = 9.805 inside, :119-121), dt to the previous
 * sample (:122).  Sample values are not checked; with a non-finite sample the output is unspecified. */
int mml_imu_preintegrate(const double* samples, int n, const double* bg, const double* ba, mml_imu_preint* out);
/* Cost_NavState_PRV_Bias (ceresfunc.h:321-393) with sqrt_information = LLT(covariance^-1).matrixL()^T
 * (Estimator.cpp:1240-1242).  pr*: [P(3), rotation vector(3)], vb*: [V(3), bg(3), ba(3)].  residual: 15;
 * jacobian (may be NULL): 15 x 30 row-major, columns [pr_i | vb_i | pr_j | vb_j]. */
int mml_imu_factor(const mml_imu_preint* pre, const double* gravity, const double* pr_i, const double* vb_i,
                   const double* pr_j, const double* vb_j, double* residual, double* jacobian);
/* MarginalizationFactor living on (para_PR[0], para_VBias[0]) (ceresfunc.h:244-303): residual =
 * r0 + J * dx(x, x0) with the reference's dx (translation / velocity / bias differences, rotation part
 * log(exp(x)^-1 exp(x0)), :274-283); J is handed to the solver unchanged. */
typedef struct {
    double J[225];            /* linearized_jacobians, 15 x 15 row-major, columns [PR 6 | VBias 9] */
    double r0[15];            /* linearized_residuals */
    double x0[15];            /* keep_block_data */
} mml_prior;
typedef struct mml_fullwindow mml_fullwindow;
/* Estimator::Estimate in full-window mode (Estimator.cpp:1226-1254,1425-1432): W frames x [PR 6 | VBias 9]. */
mml_fullwindow* mml_fullwindow_create(int W, const mml_solve_opts* opts);
void mml_fullwindow_destroy(mml_fullwindow*);
/* IMU factor between frames f-1 and f (1 <= f < W), Estimator.cpp:1235-1248. */
int mml_fullwindow_set_imu(mml_fullwindow*, int f, const mml_imu_preint* pre, const double* gravity);
/* last_marginalization_info (NULL: none), Estimator.cpp:1249-1254. */
int mml_fullwindow_set_prior(mml_fullwindow*, const mml_prior* prior);
/* One trust-region evaluation, same protocol as mml_window_solver_step: records = W x 32 lidar records evaluated at
 * x_eval (W x 15, in/out).  Returns 1 when finished, 0 when x_eval holds the next point to evaluate, < 0 on error. */
int mml_fullwindow_step(mml_fullwindow*, const double* records, double* x_eval);
int mml_fullwindow_summary(const mml_fullwindow*, mml_solve_summary* out);
/* The dense normal equations of the whole window at x (W x 15): H (15W x 15W row-major), g, cost. */
int mml_fullwindow_normal_equations(const mml_fullwindow*, const double* records, const double* x, double* H, double* g,
                                    double* cost);
/* MarginalizationInfo::marginalize for the factor set of Estimator.cpp:1453-1546 (previous prior, IMU factor 0-1,
 * lidar factors of frame 0 as their loss-free normal equations).  x: W x 15.  out: the prior for the slid window. */
int mml_fullwindow_marginalize(const mml_fullwindow*, const double* lidar_record0, const double* x, mml_prior* out);
/* ---- the LIO initialisation that opens full-window mode (TryMAPInitialization, unionPoseEstimation.cpp:425-625) ------
 * Host side like the rest of this section: no context, no device. */
/* IMUIntegrator::GyroIntegration (IMUIntegrator.cpp:90-106): the gyro samples accumulated onto dq (x, y, z, w; in/out,
 * not reset first).  samples: n x 7 as for mml_imu_preintegrate; only angular_velocity and dt are read.  A dt < 0 (the
 * reference's ROS_ASSERT) is MML_ERR_INVALID and leaves dq unchanged. */
int mml_imu_gyro_integrate(const double* samples, int n, double* dq);
/* Cost_Initialization_IMU (ceresfunc.h:654-741) with sqrt_information = LLT(covariance.block<9,9>(0,0)^-1).matrixL()^T
 * (unionPoseEstimation.cpp:558-561).  ri, rj: rotation vectors of the two body orientations; dp: body position j minus
 * body position i; rwg, vi, vj, ba, bg: the parameter blocks.  residual: 9; jacobian (may be NULL): 9 x 15 row-major,
 * columns [rwg | vi | vj | ba | bg] (analytic). */
int mml_imu_init_factor(const mml_imu_preint* pre, const double* ri, const double* rj, const double* dp, const double* rwg,
                        const double* vi, const double* vj, const double* ba, const double* bg, double* residual,
                        double* jacobian);
typedef struct {
    int status;                  /* 0 initialised; 1 |b_a| or |b_g| > 0.5 (nothing written); 2 a velocity more than 2.0
                                    from its prior (frames 0..fail_frame hold the new biases, 0..fail_frame-1 the new V);
                                    3 (mml_lio_initialize_batch only; the single call returns MML_ERR_STATE): the
                                    pre-integration of frame fail_frame has a covariance that is not positive definite,
                                    e.g. an empty interval (nothing written but status and fail_frame) */
    int fail_frame;              /* status 2, 3: that frame; -1 otherwise */
    int keep_from;               /* status 0: the caller drops frames [0, keep_from) (the list is trimmed to 5 frames) */
    int _pad;
    double gravity[3];           /* GravityVector = exp(r_wg) (0, 0, -9.805) */
    double r_wg[3];              /* the joint solve's rotation vector */
    double q_wg[4];              /* the gravity solve's quaternion, x y z w */
    double average_acc[3];       /* -GetAverageAcc() of frame 0, rescaled to norm 9.805 */
    double ba[3], bg[3];         /* the joint solve's biases (also when a check failed) */
    mml_solve_summary gravity_solve, joint_solve;   /* the two ceres::Solve calls */
} mml_lio_init_result;
/* TryMAPInitialization on n >= 2 frames (the reference's list, front first).  t: n time stamps; P (n x 3), Q (n x 4,
 * x y z w): lidar poses, world <- lidar; V, bg, ba (n x 3): the frame states, written as the reference writes them
 * (status 0: all; status 2: the partial state above; the back frame's P, Q converted to the body on status 0 only).
 * samples / offsets: frame i's IMU messages are rows offsets[i] .. offsets[i+1]-1 of an n x 7 array as for
 * mml_imu_preintegrate (frame i's first dt counts from t[i-1]); frame 0 needs at least one.  exTlb: 4 x 4 row-major.
 * pre_in (may be NULL): n entries, entry i >= 1 the pre-integration frame i holds; NULL: each is computed from its
 * samples with frame i-1's bg / ba.  pre_out (may be NULL): n entries, entry i >= 1 receives the pre-integration the
 * joint solve used, on status 0 the one redone with the new biases (entry 0 is not written).  Returns MML_OK whatever
 * the status; < 0 on a bad argument or a covariance that is not positive definite. */
int mml_lio_initialize(int n, const double* t, double* P, double* Q, double* V, double* bg, double* ba, const double* samples,
                       const int* offsets, const double* exTlb, const mml_imu_preint* pre_in, mml_imu_preint* pre_out,
                       mml_lio_init_result* out);
/* The minimisation of the mml_fullwindow_step loop with the whole trust-region iteration resident on the device: the
 * lidar factors of the W frames in slots first_slot .. first_slot + W - 1 (associated beforehand, evaluated with the
 * handle's plan_weight_tan / huber_delta), the IMU factors and the prior set on `fw` are evaluated, assembled into the
 * block-tridiagonal band of the 15 W normal equations, factored and stepped by ONE kernel launch -- no host round
 * trip per evaluation.  x: W x 15 in/out; summary / evaluations may be NULL.  Afterwards mml_fullwindow_summary
 * reports this solve and mml_fullwindow_marginalize can be called with the returned x. */
int mml_fullwindow_solve(mml_ctx* ctx, mml_fullwindow* fw, int first_slot, const double* T_bl, double* x,
                         mml_solve_summary* summary, int* evaluations);
/* n such solves in one device call: the same kernels with a window dimension, so that many windows (a fleet's bags, one
 * bag cut into segments) fill the device instead of the 2 W + 1 workgroups of one.  Window w is handle fws[w] -- its own
 * W, options, IMU factors and prior; windows may differ in all of them -- on the factor lists of slots first_slot[w] ..
 * first_slot[w] + W_w - 1 (windows may share slots: the solve only reads them), with its state in the first 15 W_w doubles
 * of x + MML_FW_X_STRIDE w (in/out) and one T_bl for all.  The rounds run to the largest max_num_iterations + 1 of the
 * batch; a window that has finished costs nothing further, and the enqueue loop stops when none is left.  Every window's
 * result is bit-identical to mml_fullwindow_solve called on it alone, and every handle is left as that call leaves it
 * (mml_fullwindow_summary, mml_fullwindow_marginalize).  summaries / evaluations: n entries or NULL.  records0 (n x 32 or
 * NULL): entry w receives the record of window w's frame 0 at the returned x, linearised with that handle's
 * plan_weight_tan and huber_delta -- what mml_linearize_window(first_slot[w], 1, ...) returns and
 * mml_fullwindow_marginalize takes -- all of them from one launch and one read-back.
 * Everything is checked before anything is enqueued and the message names the window: MML_ERR_INVALID for n < 1 or
 * n > MML_FW_BATCH_MAX, a null entry, a handle that appears twice, a window that does not fit the slots,
 * max_num_iterations outside 0 .. 1000; MML_ERR_STATE for a pre-integration whose covariance is not positive definite.
 * The context keeps device and pinned buffers for the largest n it has seen (about 0.2 MB per window). */
#define MML_FW_X_STRIDE 120   /* 15 * 8 doubles per window in x */
#define MML_FW_BATCH_MAX 1024 /* windows per call */
int mml_fullwindow_solve_batch(mml_ctx* ctx, int n, mml_fullwindow* const* fws, const int* first_slot, const double* T_bl,
                               double* x /* n x MML_FW_X_STRIDE, in/out */, mml_solve_summary* summaries /* n or NULL */,
                               int* evaluations /* n or NULL */, double* records0 /* n x 32 or NULL */);
/* mml_fullwindow_marginalize for n windows in one device call: one launch (a workgroup per window) and one read-back of
 * n priors, no lidar record fetched first.  Window w uses handle fws[w] -- its IMU factor 1, prior, gravity and
 * plan_weight_tan; the handles are only read, so one may appear more than once -- the associated factor lists of slot
 * first_slot[w] (the window's frame 0) and the state in x + MML_FW_X_STRIDE w (its first 30 doubles are read).  The lidar
 * factors are linearised WITHOUT a loss function whatever huber_delta the handle holds (the reference stores them so).
 * priors[w] is bit-identical to mml_fullwindow_marginalize(fws[w], rec, x_w, ...) with rec the record
 * mml_linearize_window(first_slot[w], 1, x_w, T_bl, plan_weight_tan, 0.0) returns: the device runs the host's operations
 * in the host's order (csrc/marg_dense.h).
 * Everything is checked before anything is enqueued and the message names the window: MML_ERR_INVALID for n < 1 or
 * n > MML_FW_BATCH_MAX, a null entry, W < 2, no IMU factor 1, a slot out of range (a NULL ctx after the handle checks);
 * MML_ERR_STATE for a pre-integration whose covariance is not positive definite.  The context keeps device and pinned
 * buffers for the largest n it has seen (about 20 KB per window). */
int mml_fullwindow_marginalize_batch(mml_ctx* ctx, int n, mml_fullwindow* const* fws, const int* first_slot, const double* T_bl,
                                     const double* x /* n x MML_FW_X_STRIDE */, mml_prior* priors /* n */);
/* mml_imu_preintegrate for n intervals in one call -- what feeds the two batch calls above.  Interval i is rows
 * offsets[i] .. offsets[i+1]-1 of samples (rows of 7 doubles as for mml_imu_preintegrate) with the linearisation biases
 * bg + 3 i, ba + 3 i; an empty interval gives the reset state (identity Jacobian, zero covariance, dq = (0, 0, 0, 1)).
 * ctx NULL: the host build of the routine (csrc/imu_preint.h) in a loop, no device needed.  Otherwise one upload, one launch
 * (a workgroup of one wavefront per interval) and one read-back; the device build runs the host's operations in the host's
 * order, so the two are bit-identical.  Against mml_imu_preintegrate the routine differs in one place: the right Jacobian
 * takes its sin / cos from the project's own kernels (csrc/imu_math.h), not from libm, so out[i] has the bytes of the single
 * call wherever no step rotates by more than 1e-5 rad, and agrees to rounding elsewhere.
 * Everything is checked before anything is enqueued or written and the message names the interval: MML_ERR_INVALID for
 * n < 1 or n > MML_PREINT_BATCH_MAX, a null pointer (samples may be NULL when offsets[n] is 0), offsets[0] != 0, a
 * decreasing offset.  Sample values are not checked, as in the single call.  The context keeps device and pinned buffers for
 * the largest call it has seen (3.7 KB per interval and 56 bytes per sample). */
#define MML_PREINT_BATCH_MAX 8192 /* intervals per call */
int mml_imu_preintegrate_batch(mml_ctx* ctx, int n, const double* samples, const int* offsets /* n + 1 */,
                               const double* bg /* n x 3 */, const double* ba /* n x 3 */, mml_imu_preint* out /* n */);
/* mml_lio_initialize for n_seg segments in one call -- what opens full-window mode for the three batch calls above.  Segment s
 * is frames frame_offsets[s] .. frame_offsets[s+1]-1 (2 .. MML_LIO_BATCH_MAX_FRAMES of them) of the concatenated arrays t, P,
 * Q, V, bg, ba (F = frame_offsets[n_seg] rows), frame f's IMU messages are rows sample_offsets[f] .. sample_offsets[f+1]-1 of
 * samples, exTlb + 16 s is the segment's extrinsic, and pre_in / pre_out (either may be NULL) hold F entries of which a
 * segment's entry 0 is not read or written.  Per segment every argument means what it means in mml_lio_initialize: the partial
 * writes of status 1 / 2, keep_from, the back frame moved to the body on status 0 only, out[s].  Where the single call fails as
 * a whole with MML_ERR_STATE (a pre-integration covariance that is not positive definite, e.g. an empty interval of a frame
 * >= 1) the segment gets status 3 and fail_frame, none of its state or pre_out entries is written, and the other segments are
 * unaffected.
 * ctx NULL: the host build of the routine (csrc/lio_init_core.h, csrc/imu_preint.h) in a loop over the segments, no device
 * needed.  Otherwise one upload, three launches (the pre-integrations a wavefront per frame, the initialisation a wavefront per
 * segment with the whole solve state in LDS, the pre-integrations again for status-0 segments with the new biases) and one
 * read-back; the device build runs the host's operations in the host's order, so the two are bit-identical on every output
 * byte.  Against mml_lio_initialize the routine differs in the two places where that call reaches libm: the quaternion step
 * of the gravity solve takes its sin / cos from csrc/imu_math.h, and the pre-integrations are mml_imu_preintegrate_batch's.
 * Both agree with libm to an ulp: results agree to rounding amplified by the solves (1e-9 in the tests).
 * Everything is checked before anything is enqueued or written and the message names the segment: MML_ERR_INVALID for n_seg
 * outside 1 .. MML_LIO_BATCH_MAX, a null pointer (pre_in / pre_out may be NULL), frame_offsets[0] != 0, a segment with fewer
 * than 2 or more than MML_LIO_BATCH_MAX_FRAMES frames, sample_offsets[0] != 0, a decreasing sample offset, a segment whose
 * frame 0 has no sample.  The context keeps one device and one pinned block for the largest call it has seen (3.8 KB per frame
 * and 56 bytes per sample). */
#define MML_LIO_BATCH_MAX        1024   /* segments per call */
#define MML_LIO_BATCH_MAX_FRAMES 8      /* frames per segment (2 .. 8) */
int mml_lio_initialize_batch(mml_ctx* ctx, int n_seg, const int* frame_offsets /* n_seg + 1 */,
        const double* t, double* P, double* Q, double* V, double* bg, double* ba,      /* F rows, F = frame_offsets[n_seg] */
        const double* samples, const int* sample_offsets /* F + 1 */,
        const double* exTlb /* n_seg x 16 */, const mml_imu_preint* pre_in /* F or NULL */,
        mml_imu_preint* pre_out /* F or NULL */, mml_lio_init_result* out /* n_seg */);

/* ---- the pose node's IMU queue: a device-resident message store cut and pre-integrated per frame interval -------------------
 * What produces the samples / offsets arrays the batch calls above start from.  A mml_imu_stream is _imuMsgVector
 * (unionPoseEstimation.cpp:296) in device memory: rows of 7 doubles = header.stamp.toSec(), angular_velocity xyz,
 * linear_acceleration xyz as in the message (not yet * gnorm).  Messages are counted absolutely over everything ever pushed:
 * `front` is the first live one, `tail` one past the last.  Housekeeping as for mml_livox_stream: the stream belongs to its
 * context and is destroyed before it; push is one host-to-device copy and one kernel, asynchronous on the context's stream (the
 * host buffer must stay valid until the next synchronising call); MML_ERR_CAPACITY, changing nothing, when the live messages plus
 * n exceed capacity_msgs (1 .. 2^24); when the array's end is reached the live part moves to the front of a second array (one
 * device-to-device copy on the stream), so a stream holds 112 bytes per message of capacity.
 * The host keeps a mirror of the stamps (8 bytes per message, written at push), so mml_imu_stream_drop_before -- the trim of
 * :383-390: while live > keep_min and stamp[front] < t: ++front; the reference has keep_min = 200 and
 * t = min(_time_last_hori, _time_last_velo) -- and the stamps of mml_imu_stream_state_get need no device work and no
 * synchronisation; state_get synchronises once, for `disorder`.
 * TIME ORDER.  The cut needs stamps that do not decrease, across pushes too; equal stamps are allowed.  The push kernel counts
 * the violations (`disorder`, each message compared with the one before it in the queue); mml_imu_fetch_batch refuses a stream
 * that has any.  What the reference does with unordered stamps depends on the order of its walk and is not reproduced.
 * mml_imu_stream_reset empties the stream and forgets the violations. */
typedef struct mml_imu_stream mml_imu_stream;
int  mml_imu_stream_create(mml_ctx* ctx, long capacity_msgs, mml_imu_stream** out);
void mml_imu_stream_destroy(mml_imu_stream* s);
int  mml_imu_stream_reset(mml_imu_stream* s);
int  mml_imu_stream_push(mml_imu_stream* s, const double* msgs /* n x 7 */, int n);
int  mml_imu_stream_drop_before(mml_imu_stream* s, double t, long keep_min);
typedef struct { long front, tail; long disorder; double first_stamp, last_stamp; /* of the live messages; 0 when none */ } mml_imu_stream_state;
int  mml_imu_stream_state_get(mml_imu_stream* s, mml_imu_stream_state* out);

/* fetchImuMsgs (unionPoseEstimation.cpp:307-395, called at :719 for every scan) for n intervals (t_start[i], t_end[i]] in one
 * call, with what process() does to the result at :741-828: the cut, the message synthesised at t_end, the dt column,
 * PreIntegration with the interval's biases and GyroIntegration from the identity.  The rules, with the reference's lines, are
 * in csrc/imu_fetch.h; in short, with T the live stamps:
 *   status 1 EMPTY no live message | 4 REVERSED t_end < t_start | 2 NOT_REACHED T[tail-1] < t_end | 3 TOO_OLD T[front] >= t_end
 *   (checked in that order) | 0 OK | 5 NO_SAMPLE: the interpolation branch is reached with no message inside, where the
 *   reference reads back() of an empty vector -- defined here, n = 0; t_end == t_start always lands here.
 *   OK: the messages with t_start < T <= t_end up to the first one at t_end exactly; when none is at t_end, one more row
 *   interpolated linearly between the last message inside and the first one past the end (interpolated = 1).  A message at
 *   exactly t_start is out.  The synthesised message's stamp is t_end itself: the reference rounds it to whole nanoseconds
 *   (ros::Time::fromSec), the identity for stamps of ROS headers at epoch scale and the one deliberate difference otherwise.
 * samples: the rows of all intervals packed in order, interval i at rows offsets[i] .. offsets[i+1]-1, in the shape
 * mml_imu_preintegrate takes (gyro xyz, accel xyz, dt; row 0's dt counts from t_start).  pre[i] has the bytes of
 * mml_imu_preintegrate_batch on those rows with bg + 3 i, ba + 3 i (the same kernel, launched on the packed rows); dq[i]
 * (x, y, z, w) is GyroIntegration from the identity (the chain of mml_imu_gyro_integrate).  An interval whose status is not 0
 * has n = 0, the reset state in pre and dq = (0, 0, 0, 1).  The stream is only read: intervals may overlap or repeat.
 * sample_capacity bounds the total row count whether samples is NULL (the rows stay on the device, for pre / dq) or not.  When the
 * total exceeds it the call returns MML_ERR_CAPACITY with rows and offsets written (offsets[n] is the size needed, saturating
 * at INT_MAX) and samples, pre and dq NOT written.  With samples, pre and dq all NULL it is ignored: a sizing call.
 * Work per call, whatever n is: one upload, a plan kernel (a lane per interval: two binary searches, status, count), an
 * exclusive scan of the counts in one workgroup, a write kernel (a wavefront per interval), k_imu_preintegrate, a gyro kernel
 * (a lane per interval), one read-back -- it moves sample_capacity rows at most, so size it tightly -- and ONE host
 * synchronisation.  The device runs the host's operations in the host's order: every output byte equals mml_imu_fetch_host's.
 * Everything is checked before anything is enqueued and the message names the interval: MML_ERR_INVALID for n outside
 * 1 .. MML_IMU_FETCH_BATCH_MAX, a NULL stream, t_start, t_end, rows or offsets, a stream of another context, exactly one of bg /
 * ba NULL, pre without biases, a negative sample_capacity, a non-finite time.  MML_ERR_STATE, from the call's one read-back and
 * with nothing written, for a stream with time-order violations.  The context keeps one device and one pinned block for the
 * largest call it has seen (3.9 KB per interval and 56 bytes per row of sample_capacity), released by mml_destroy. */
typedef struct {
    int status, n;            /* rows emitted, the synthesised one included */
    long first;               /* absolute index of row 0's message; front when n == 0 */
    int interpolated, _pad;
    double front_gyro_z, back_gyro_z;   /* vimuMsg.front() / back()->angular_velocity.z, the operands of :747, :771; 0 when n == 0 */
} mml_imu_interval;
#define MML_IMU_FETCH_BATCH_MAX 8192    /* = MML_PREINT_BATCH_MAX */
int mml_imu_fetch_batch(mml_ctx* ctx, mml_imu_stream* s, int n, const double* t_start, const double* t_end,
        const double* bg, const double* ba /* n x 3 each, or both NULL: no pre-integration */,
        mml_imu_interval* rows /* n */, int* offsets /* n + 1 */, double* samples /* sample_capacity x 7 or NULL */,
        long sample_capacity, mml_imu_preint* pre /* n or NULL */, double* dq /* n x 4 or NULL */);
/* The same on a host array of messages (n_msgs x 7 as pushed, all of them live, first = 0-based row), no context, no device.
 * MML_ERR_STATE for decreasing stamps; MML_ERR_INVALID also for n_msgs outside 0 .. 2^24, NULL msgs with n_msgs > 0 or a stamp
 * that is not finite (which mml_imu_stream_push refuses too). */
int mml_imu_fetch_host(const double* msgs, long n_msgs, int n, const double* t_start, const double* t_end,
        const double* bg, const double* ba, mml_imu_interval* rows, int* offsets, double* samples, long sample_capacity,
        mml_imu_preint* pre, double* dq);
/* The frame prediction of process() for n intervals, from the results above.  exTlb: one 4 x 4, row-major (exRbl / exPbl are its
 * inverse's rotation and translation).  With prev (n x 10: the previous frame's body state P(3), Q(4, x y z w), V(3)) and pre
 * (n), :805-828: state (n x 10) = P + Q * dp, Q * dq, V + Q * dv; delta_Rl (n x 9, row-major) = Qwlpre^* Qwl and delta_tl (n x 3)
 * = Qwlpre^* (Pwl - Pwlpre), laid out as mml_step / mml_undistort take dR and dt.  With dq (n x 4), the bring-up branch :779-780:
 * gyro_Rb (n x 9) = dq.toRotationMatrix(), gyro_Rl (n x 9) = R_lb gyro_Rb R_lb^T.  Either group may be left out (all its
 * pointers NULL).  ctx NULL: the host build of csrc/imu_fetch.h; otherwise one upload, one kernel (a lane per interval), one
 * read-back, bit-identical to it.  Against the reference the quaternion products are held to rounding, not to bytes (Eigen's
 * operation order is not restated).  MML_ERR_INVALID for n outside 1 .. MML_IMU_FETCH_BATCH_MAX, NULL exTlb, a group given in part,
 * or neither group. */
int mml_imu_predict_batch(mml_ctx* ctx, int n, const double* exTlb, const double* prev, const mml_imu_preint* pre,
        double* state, double* delta_Rl, double* delta_tl, const double* dq, double* gyro_Rb, double* gyro_Rl);

/* ---- the pose node's way in: `count` union_cloud messages into scan slots in one call --------------------------------------
 * mml_cloud_upload for `count` messages at once, with the decision the pose node takes per message
 * (unionPoseEstimation.cpp:719-773) taken by the library: the mirror image of mml_feature_clouds_download_batch.  `clouds` /
 * `n_points` (count x 6) are exactly what that call returns -- slot-major, six clouds per frame in union_cloud.msg order, 48-byte
 * records, contiguous; only clouds 2 (velo_combine) and 5 (livox_combine) are read as points, and n_points[6 i + 3] is the
 * frame's livox_corner_num.  `rows` are the rows mml_imu_fetch_batch writes for the frames' intervals (n, front_gyro_z and
 * back_gyro_z are read), or NULL for IMU_Mode == 0, where vimuMsg stays empty.  Frame i goes to slot first_slot + i.
 * THE RULES (csrc/pose_ingest.h, one routine; the device call's decisions are computed on the host by the very routine behind
 * mml_pose_ingest_plan -- the device only decodes).  For frame i, in this order:
 *   DROPPED    rows given and rows[i].n == 0: fetchImuMsgs returns !vimuMsg.empty(), the reference retries, pops the message and
 *              continues (:719-730).  The slot is not touched at all; n_points = n_velo = 0; reason = MML_INGEST_WHY_FETCH + the
 *              row's fetch status.  (A dropped frame does not pass `first_frame` on: the caller names the first frame.)
 *   VELO_ONLY  without the gate: rows == NULL (reason NO_IMU), or i == opts->first_frame (first_velo_frame, :741, :838-839;
 *              reason FIRST_FRAME).  fast_rotation = 0.
 *   otherwise (:746-773), abs being std::abs(double) -- the reference's unqualified call, DESIGN.md section 2 convention 14:
 *     MERGED iff !velo_only_mode && (abs(front_gyro_z) < hori_rotate_th || abs(back_gyro_z) < hori_rotate_th) &&
 *     livox_corner_num > 100; else VELO_ONLY with the first failing test of that order as the reason (VELO_ONLY_MODE,
 *     FAST_ROTATION, FEW_CORNERS).  fast_rotation = abs(front) > velo_rotate_th || abs(back) > velo_rotate_th (:771), whatever
 *     the decision.  A NaN gyro value fails every comparison, as in the reference.
 * A MERGED slot holds velo_combine followed by livox_combine (:756); a VELO_ONLY slot velo_combine alone (n_velo == n_points).
 * The row's n_points / n_velo are what went into the slot.  Afterwards a slot is in the state mml_cloud_upload leaves, byte for
 * byte, and a dropped frame's slot -- its host-side state too -- is as it was.
 * Work per call, whatever `count` is: one host-to-device copy of the block, one table upload (32 bytes per frame), one launch of
 * the decode kernel over all frames (records loaded as whole 16-byte words, turned into points through LDS), one launch of the
 * label-list kernel over the run of slots -- one per run of adjacent slots when dropped frames split it -- and ONE host
 * synchronisation.  Synchronous like mml_cloud_upload.
 * Everything is checked before anything is enqueued, the message names the frame, and a refusal writes nothing, on the host or on
 * the device: MML_ERR_INVALID for a slot range outside the context, count < 1 or above 65535, NULL n_points / opts / out, NULL
 * clouds with a non-zero total, a negative count (in n_points or rows[i].n), first_frame outside -1 .. count-1;
 * MML_ERR_CAPACITY for a frame whose Velodyne part exceeds max_velo_points or whose MERGED Livox part exceeds max_livox_points (a
 * Livox cloud that is not taken is not measured).  The context keeps a device and a pinned table block for the largest call it
 * has seen, released by mml_destroy. */
typedef struct {
    double hori_rotate_th, velo_rotate_th;  /* 0.3, 1.5: unionPoseEstimation.cpp:146-147 (main() falls back to 0.5 for the
                                               first when ~hori_rotate_threshold is not set, :1405-1406) */
    int velo_only_mode;                     /* 0 (:85) */
    int first_frame;                        /* index of the frame that meets first_velo_frame == true, -1: none */
} mml_pose_ingest_opts;
void mml_pose_ingest_opts_default(mml_pose_ingest_opts* opts);
enum { MML_INGEST_VELO_ONLY = 0, MML_INGEST_MERGED = 1, MML_INGEST_DROPPED = 2 };   /* mml_pose_ingest_row.decision */
enum {                                                                              /* mml_pose_ingest_row.reason */
    MML_INGEST_WHY_MERGED = 0,          /* every test of :746-748 passed */
    MML_INGEST_WHY_NO_IMU = 1,          /* rows == NULL: vimuMsg.empty() at :741 */
    MML_INGEST_WHY_FIRST_FRAME = 2,     /* first_velo_frame at :741 */
    MML_INGEST_WHY_VELO_ONLY_MODE = 3,  /* :746, :767 */
    MML_INGEST_WHY_FAST_ROTATION = 4,   /* :747, :763-765 */
    MML_INGEST_WHY_FEW_CORNERS = 5,     /* :748, :760-761 */
    MML_INGEST_WHY_FETCH = 16           /* DROPPED: + rows[i].status, the fetch status 0 .. 5 of mml_imu_fetch_batch */
};
typedef struct { int decision, reason, fast_rotation, n_points, n_velo, _pad; } mml_pose_ingest_row;
/* Host only, no context: the decisions alone (and the counts they imply).  The argument checks of the device call that need no
 * context; no capacity is checked. */
int mml_pose_ingest_plan(int count, const int* n_points /* count x 6 */, const mml_imu_interval* rows /* count or NULL */,
                         const mml_pose_ingest_opts* opts, mml_pose_ingest_row* out /* count */);
int mml_pose_ingest_batch(mml_ctx* ctx, int first_slot, int count, const uint8_t* clouds, const int* n_points /* count x 6 */,
                          const mml_imu_interval* rows /* count or NULL */, const mml_pose_ingest_opts* opts,
                          mml_pose_ingest_row* out /* count */);

/* ---- the feature node's way in: `count` union_cloud messages in wire form into scan slots in one call ------------------------
 * mml_scan_upload_wire for `count` messages at once (a feature node in a process of its own, a bag reader that replays recorded
 * aligner output).  Frame i goes to slot first_slot + i.
 *   Velodyne part  frame i is n_velo[i] records of point_step bytes from byte velo_at[i] of velo_data; point_step and the field
 *                  offsets are shared by the call and mean what they mean for mml_scan_upload_pointcloud2, with its limits
 *                  (12 <= point_step <= 256, every field inside the record, off_intensity < 0: intensity 0).
 *   Livox part     frame i is n_livox[i] records of livox_record_bytes from byte livox_at[i] of livox_data: 19 = the wire form of
 *                  mml_scan_upload_wire (_pad is written as 0), 20 = mml_livox_point as it stands, pad byte included, as
 *                  mml_scan_upload copies it.
 * A sensor's offsets never decrease and its payloads never overlap: frame i starts at or behind the last byte of frame i - 1 (an
 * empty frame's offset counts).  GAPS ARE ALLOWED, so the offsets can point into one mapped bag chunk with the message headers
 * between the payloads.  Per sensor the call copies ONE span, from the first payload's first byte to the last payload's last
 * byte: the gaps travel too, and a caller whose payloads are far apart pays for the bytes between them.  Either part of any
 * frame may be empty; a sensor without any point may pass NULL for its data pointer (and for its offsets).
 * Afterwards every slot is exactly what mml_scan_upload_wire (19) / mml_scan_upload_pointcloud2 (20) leaves on that frame alone:
 * the rows of the raw buffers, the counts on the device and on the host, and the slot counts as not extracted.
 * Asynchronous on the context's stream like the single calls, and the host buffers must stay valid until the next synchronising
 * call.  Work per call, whatever `count` is: at most two payload copies, one table copy (32 bytes per frame), ONE launch of the
 * decode kernel over (sensor, frame, tile of 256 points), one copy of the counts.  No host synchronisation (the staging buffer grows to the
 * largest call, and a growth waits for the stream, as for the single calls).
 * Everything is checked before anything is enqueued; a refusal names the frame in mml_last_error and changes nothing, on the host
 * or on the device: MML_ERR_INVALID for a slot range outside the context, count < 1 or above 65535, NULL count arrays, a bad
 * point_step / field offset / livox_record_bytes, a negative count or offset, an offset before the end of the frame before it,
 * NULL data or offsets with points announced; MML_ERR_CAPACITY for a frame above max_velo_points / max_livox_points. */
int mml_scan_upload_wire_batch(mml_ctx* ctx, int first_slot, int count, const uint8_t* velo_data, const int64_t* velo_at,
                               const int* n_velo, int point_step, int off_x, int off_y, int off_z, int off_intensity,
                               const uint8_t* livox_data, const int64_t* livox_at, const int* n_livox, int livox_record_bytes);
/* Host only, no context: the argument rules of the call above (csrc/wire_decode.h, the routine the device call runs), with the
 * capacities given by the caller (negative: not checked).  MML_OK: span = the bytes the call would copy, as half-open ranges --
 * span[0] the Velodyne span's first byte, span[1] one past its last byte, span[2] / span[3] the same for the Livox span; 0, 0 for
 * a sensor without points.  Otherwise span is untouched.  *bad_frame (may be NULL): the frame a refusal is about, -1 when it is
 * about the call as a whole or there is none. */
int mml_scan_upload_wire_plan(int count, const int64_t* velo_at, const int* n_velo, int point_step, int off_x, int off_y, int off_z,
                              int off_intensity, const int64_t* livox_at, const int* n_livox, int livox_record_bytes,
                              int max_velo_points, int max_livox_points, int64_t span[4], int* bad_frame);
/* The decode itself on the host, for callers without a device: the same arguments and rules (no capacity), frame i's Velodyne
 * points as x, y, z, intensity from row sum(n_velo[0 .. i)) of velo_xyzi, its Livox points from row sum(n_livox[0 .. i)) of
 * livox.  Bit patterns are moved, never computed with. */
int mml_wire_decode_host(int count, const uint8_t* velo_data, const int64_t* velo_at, const int* n_velo, int point_step, int off_x,
                         int off_y, int off_z, int off_intensity, const uint8_t* livox_data, const int64_t* livox_at,
                         const int* n_livox, int livox_record_bytes, float* velo_xyzi, mml_livox_point* livox);

/* Number of HIP streams mml_step pipelines its sub-batches over (1..8, default 2 or $MML_LANES).  With 1 every
 * kernel covers the whole batch and runs alone on the device, which is what per-kernel timing wants. */
int mml_set_lanes(mml_ctx* ctx, int lanes);
int mml_profile_enable(mml_ctx* ctx, int on);
int mml_profile_reset(mml_ctx* ctx);
int mml_profile_get(mml_ctx* ctx, mml_profile* out);
/* How many points of a slot's last extraction left the fast path: `redo` = points whose float pre-decision of an angle
 * predicate fell inside its guard band and were recomputed with the full decision chain (k_stencil_redo), `brk` = break-point
 * candidates finished by k_stencil_break (unionFeatureExtract.cpp:651-806).  Either may be NULL. */
int mml_extract_queue_counts(mml_ctx* ctx, int slot, int* redo, int* brk);
/* Test hook: the device's copies of the two libm routines the ring / azimuth assignment calls (csrc/libm_f32.h: glibc's atanf and
 * atan2f, the float overloads unionFeatureExtract.cpp:1136-1139,1159,1168 resolve to), evaluated on n host values on the
 * context's device.  out_atan2[i] = atan2f(y[i], x[i]), out_atan[i] = atanf(y[i]); either output may be NULL. */
int mml_libm_f32(mml_ctx* ctx, const float* y, const float* x, long n, float* out_atan2, float* out_atan);
/* Test hook: the device's own model-fit code (the __device__ functions the association and GICP kernels call) on n
 * caller-supplied items, one lane per item, on the context's device.  Per item, by operation code:
 *   MML_FIT_EIG3    in  6 doubles m00 m10 m11 m20 m21 m22 (lower triangle)
 *                   out 12 doubles: eigenvalues ascending, then the eigenvectors of ev[0], ev[1], ev[2]
 *   MML_FIT_QR      in  15 doubles, 5 x 3 row-major;  out 4 doubles: X[3] of the column-pivoted QR solve of A X = -1, rank
 *   MML_FIT_LINE    in  15 floats, the 5 neighbours in search order
 *                   out 13 doubles: accepted (0 / 1), centroid[3], ev[3], p1[3], p2[3] (the float values as stored)
 *   MML_FIT_PLANE   in  18 floats, the 5 neighbours and the selected point
 *                   out 11 doubles: accepted, X[3], pa pb pc pd (floats), proj[3]
 *   MML_FIT_OPS_F64 in  2 doubles a b;  out 2 doubles sqrt(a), a / b
 *   MML_FIT_OPS_F32 in  2 floats a b;   out 2 floats sqrtf(a), a / b
 * p1 / p2 and proj of a rejected model are never computed and come back as 0.  Codes from 6 on are free. */
enum { MML_FIT_EIG3 = 0, MML_FIT_QR = 1, MML_FIT_LINE = 2, MML_FIT_PLANE = 3, MML_FIT_OPS_F64 = 4, MML_FIT_OPS_F32 = 5 };
int mml_model_fit5(mml_ctx* ctx, int op, const void* in, long n, void* out);
/* Test hook: the dense tail of the marginalization (csrc/marg_dense.h: eigen-decomposition of the marginalized block, Schur
 * complement, square-root form) on n caller-supplied systems.  A: n x 900 (30 x 30 row-major, the first 15 parameters are
 * marginalized), b: n x 30; J: n x 225, r0: n x 15.  ctx NULL: the host build of the routine, what
 * mml_fullwindow_marginalize runs (no device needed); otherwise the device build, one workgroup of one wavefront per item.
 * The two are bit-identical. */
int mml_marginalize_dense(mml_ctx* ctx, long n, const double* A, const double* b, double* J, double* r0);
/* Test hook: the trust-region state machine of the lidar solves (csrc/solve.hip) replayed on n scripts of records given in
 * advance (open loop: the records are no function of the candidate).  Per script hdr holds W (1..8), fixed, max_iters, R
 * (1..rounds_max); x0: n x 48; records: n x rounds_max x 8 x 28 (per frame the 21 upper entries of H, g, cost).  Round 0
 * initialises from the records at x0, round r >= 1 accepts or rejects on the records of the r-th candidate; every round then
 * proposes until a candidate needs evaluating or the machine stops (rounds after that change nothing).
 * variant 0: host tr_propose / tr_decide, what mml_window_solver_step runs (ctx may be NULL);  1: the same two on one device lane;
 * 2: tr_propose_w1_wave / tr_decide_wave (k_solve, W = 1);  3: tr_propose_w1_regs / tr_decide_w1_regs (k_solve_wide);
 * 4: tr_propose_wave / tr_decide_wave (the frame-parallel window solve).  2 and 3 refuse W != 1.  One workgroup per script.
 * Per round: xc (n x rounds_max x 48: the candidate, or x once stopped), digest (MML_TR_DIGEST_DOUBLES: cost, radius, mu, alpha,
 * dogleg_norm, model_change, step_norm, x_norm, x[48]) and digest_i (MML_TR_DIGEST_INTS: iter, successful, num_invalid, reuse,
 * termination, go, evaluate, the MML_TR_D_* code of the decision (0: none), the number of proposals of the round, the branch
 * codes of the first five, 2 spare).  A branch code is one of the MML_TR_* values below + 16 x (the number of times the solve
 * raised mu inside the call) + MML_TR_FAILED if the call was the fifth invalid step in a row. */
enum {
    MML_TR_GAUSS_NEWTON = 1, MML_TR_CAUCHY = 2, MML_TR_INTERP_NEG = 3 /* c <= 0 */, MML_TR_INTERP_POS = 4 /* c > 0 */,
    MML_TR_SOLVE_FAILED = 5, MML_TR_MODEL_INVALID = 6, MML_TR_STOP_ITER = 8, MML_TR_STOP_RADIUS = 9, MML_TR_FAILED = 256
};
enum {
    MML_TR_D_PARAMETER_TOL = 1, MML_TR_D_FUNCTION_TOL = 2, MML_TR_D_GRADIENT_TOL = 3, MML_TR_D_REJECTED = 4,
    MML_TR_D_ACCEPT_SHRINK = 5 /* rel < 0.25 */, MML_TR_D_ACCEPT_KEEP = 6, MML_TR_D_ACCEPT_GROW = 7 /* rel > 0.75 */
};
#define MML_TR_DIGEST_DOUBLES 56
#define MML_TR_DIGEST_INTS 16
int mml_debug_tr_replay(mml_ctx* ctx, int variant, int n, int rounds_max, const int* hdr, const double* x0, const double* records,
                        double* xc, double* digest, int* digest_i);
/* Test hook: the trust-region state machine of the full-window (IMU_Mode 2) solve replayed on n scripts of normal equations
 * given in advance (open loop), the full-window analogue of mml_debug_tr_replay with its round semantics and its codes.
 * hdr: n x 4 (W 1..8, fixed 0/1, max_iters 0..1000, R 1..MML_FW_REPLAY_ROUNDS_MAX); x0: n x 120 (the first 15 W used).  Rounds are
 * packed raggedly: round r of script s starts at rounds[offsets[s] + r (46 m + 1)], m = 15 W, and holds the band of H as k_fw_step
 * keeps it (m x 45: row a, band column c stands for column 15 (a / 15 - 1) + c; band columns outside 0 .. m - 1 are ignored),
 * g (m) and the cost.  rounds_len: the doubles in rounds.  Refused with MML_ERR_INVALID before anything is allocated or launched:
 * n outside 0..MML_FW_REPLAY_SCRIPTS_MAX, a header value out of range, a null array, a script that does not lie inside rounds,
 * more than 64 MB of rounds, variant 1 without a context.
 * variant 0: the host's propose / decide and the initialisation of mml_fullwindow_step (csrc/window_imu.hip; ctx may be NULL), the
 * dense H being the band with exact zeros outside it;  1: the device's fw_round -- what k_fw_step runs once the equations are
 * assembled: initialisation, fw_decide, fw_propose with fw_factor_solve -- one workgroup per script.
 * Outputs are per round, the rounds of script s at rows sum(R of the scripts before s) + r: xc (rows x 120: the candidate, or x
 * once stopped), digest (rows x MML_FW_DIGEST_DOUBLES: cost, radius, mu, alpha, dogleg_norm, model_change, step_norm, x_norm,
 * x[120]) and digest_i (rows x MML_TR_DIGEST_INTS, the layout and the codes of mml_debug_tr_replay). */
#define MML_FW_DIGEST_DOUBLES 128
#define MML_FW_REPLAY_ROUNDS_MAX 256
#define MML_FW_REPLAY_SCRIPTS_MAX 1024
int mml_debug_fw_replay(mml_ctx* ctx, int variant, int n, const int* hdr, const double* x0, const long long* offsets,
                        const double* rounds, long long rounds_len, double* xc, double* digest, int* digest_i);
/* Test hook: the pieces of the device's GICP (csrc/gicp.hip) on caller-supplied inputs -- the kernels and __device__ functions the
 * alignments run, not copies.  Clouds are n x 3 floats, covariances and Mahalanobis matrices n x 9 doubles (row-major 3 x 3),
 * a state is x = (t, roll, pitch, yaw) in 6 doubles, T is a row-major 4 x 4 float matrix.  By operation code:
 *   MML_GICP_DBG_COV    in  tgt (n_tgt >= 20 points: the cloud)
 *                       out out_d n x 9: the covariances;  out_i n x 20: every point's neighbour ids in the order of k_gicp_cov's list
 *   MML_GICP_DBG_CORR   in  src, tgt, cov_src, cov_tgt, T, gate2 (<= 0: no gate)
 *                       out out_i n_src: corr (-1: gated out);  out_d n_src x 9: maha (zeros where corr = -1)       [k_gicp_corr]
 *   MML_GICP_DBG_EVAL   in  src, tgt, corr, maha, x (k states), grad (0 / 1), gate2 (> 0: corr may hold -1, as after a gated k_gicp_corr)
 *                       out out_d k x 2 x 7: f and g[6] (zeros without grad) as lane 0 holds them, then as the workgroup's last lane does
 *                       [one workgroup as k_gicp_bfgs's calling gicp_eval]
 *   MML_GICP_DBG_INTERP in  x: k x 8 doubles (a, fa, fpa, b, fb, fpb, xmin, xmax; fpb NaN: the quadratic);  out out_d k: interpolate
 *   MML_GICP_DBG_QUAD   in  x: k x 3 doubles (a, b, c);  out out_d k x 3: the root count and the two roots (0 where there is none) of solve_quadratic
 *   MML_GICP_DBG_STATE  in  x: k states;  out out_f k x 16: apply_state;  out_d k x 6: the state k_gicp_bfgs's opening recovers from that matrix
 *   MML_GICP_DBG_ROUND  in  src, tgt, corr, maha, T, gate2, max_iterations, transformation_epsilon
 *                       out the state after ONE launch of k_gicp_bfgs from {T, nr = 0}: out_f 16: T;  out_i 4: converged, failed, nr, evals;
 *                       out_d 2: fobj, delta.  converged = (nr >= max_iterations || delta < 1), delta = the largest |T_in - T_out| entry
 *                       over 2e-3 (rotation block) or transformation_epsilon (elsewhere); fewer than 4 kept correspondences: failed = 1,
 *                       T as it came in.
 * Refused with MML_ERR_INVALID before anything is allocated or launched: an unknown op, a null array the op reads or writes, COV
 * with fewer than 20 points, any other cloud of fewer than 1 point, more than MML_GICP_DBG_MAX_POINTS points in a cloud, k outside
 * 1 .. MML_GICP_DBG_MAX_ITEMS, a corr entry outside -1 .. n_tgt - 1 (or -1 without a gate), EVAL with no correspondence, ROUND with
 * max_iterations < 1 or a transformation_epsilon that is not positive and finite.  Fields an op does not name are ignored. */
enum {
    MML_GICP_DBG_COV = 0, MML_GICP_DBG_CORR = 1, MML_GICP_DBG_EVAL = 2, MML_GICP_DBG_INTERP = 3, MML_GICP_DBG_QUAD = 4,
    MML_GICP_DBG_STATE = 5, MML_GICP_DBG_ROUND = 6
};
#define MML_GICP_DBG_MAX_POINTS (1 << 20)
#define MML_GICP_DBG_MAX_ITEMS  (1 << 20)
typedef struct mml_gicp_debug {
    const float* src;  const float* tgt;
    const double* cov_src;  const double* cov_tgt;
    const float* T;
    const int* corr;  const double* maha;
    const double* x;
    double* out_d;  int* out_i;  float* out_f;
    double gate2, transformation_epsilon;
    int n_src, n_tgt, k, grad, max_iterations, _pad;
} mml_gicp_debug;
int mml_debug_gicp(mml_ctx* ctx, int op, const mml_gicp_debug* io);
/* How many 5-NN queries of the context's last association call (mml_associate / mml_step's association on the lane that ran
 * last) went beyond rings 0-1 of the grid into the far-query kernels (k_associate_hard): the share to watch when the map's density
 * and the configured cell edge do not fit each other. */
int mml_associate_far_count(mml_ctx* ctx, int* n);
/* Device facts for bench.py: name, CU count, total HBM bytes. */
int mml_device_info(mml_ctx* ctx, char* name, int name_cap, int* cus, size_t* hbm_bytes);
/* Device-to-device copy bandwidth probe (GB/s, read + write counted) over `bytes` bytes, `reps` repetitions: the better of a
 * grid-stride 16-byte copy and a non-temporal one with four loads in flight per lane (the practical HBM roof). */
int mml_copy_bandwidth(mml_ctx* ctx, size_t bytes, int reps, double* gbps);
/* Instruction-issue probe for bench.py's `issue` object: wave64 instructions per second the whole device sustains on eight
 * independent chains per lane at eight wavefronts per SIMD.  kind 0: v_fma_f32 (every float / VOP3 instruction class measured
 * issues at this rate, 4 cycles per wavefront: tools/issue_probe.hip, profiles/r06_issue_probe.txt); kind 1: v_add_u32 (simple
 * 32-bit integer VOP2 instructions, about twice that). */
int mml_issue_rate(mml_ctx* ctx, int kind, int reps, double* wave_instr_per_s);

#ifdef __cplusplus
}
#endif
#endif /* MMLOAM_HIP_H */
