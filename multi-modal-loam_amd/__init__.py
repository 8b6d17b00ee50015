"""multi-modal-loam_amd -- MI355X-native scan-registration hot path of TIERS/multi-modal-loam.

This package is a thin ctypes view of the C-ABI in include/mmloam_hip.h (libmmloam_hip.so, built from
csrc/*.hip for gfx950).  It exists for the pytest harness, bench.py and Python users; the C++ adapter that
mirrors the reference classes (feature_extraction / Estimator) is host/mmloam_adapter.hpp.

There is no CPU fallback: importing works without a GPU (so the symbol-export test can run), but creating a
Context without a HIP device raises MmlError(MML_ERR_NO_DEVICE).

Import with importlib.import_module("multi-modal-loam_amd") (the directory name is not a Python identifier).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MML_LIB_PATH") or os.path.join(_HERE, "libmmloam_hip.so")   # ($MML_LIB_PATH: an A/B build of the library)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mmloam_hip.h")

MML_OK, MML_ERR_INVALID, MML_ERR_NO_DEVICE, MML_ERR_HIP, MML_ERR_CAPACITY, MML_ERR_STATE = 0, -1, -2, -3, -4, -5
NEQ_RECORD_DOUBLES = 32
MAX_STAGES = 32
DIGEST_WORDS = 10
FW_X_STRIDE = 120      # MML_FW_X_STRIDE: doubles per window in the state array of mml_fullwindow_solve_batch
FW_BATCH_MAX = 1024     # MML_FW_BATCH_MAX: windows per call
PREINT_BATCH_MAX = 8192  # MML_PREINT_BATCH_MAX: intervals per call of mml_imu_preintegrate_batch
LIO_BATCH_MAX = 1024     # MML_LIO_BATCH_MAX: segments per call of mml_lio_initialize_batch
LIO_BATCH_MAX_FRAMES = 8  # MML_LIO_BATCH_MAX_FRAMES: frames per segment
TOFS_BATCH_MAX = 65535    # MML_TOFS_BATCH_MAX: problems per call of mml_time_offset_search_batch
GICP_BATCH_MAX = 65535    # MML_GICP_BATCH_MAX: problems / slots per call of mml_gicp_align_batch / mml_gicp_refresh_batch
UNION_BATCH_MAX = 65535   # MML_UNION_BATCH_MAX: frames per call of mml_union_assemble
FOV_BATCH_MAX = 65535     # MML_FOV_BATCH_MAX: frames per call of mml_velo_fov_select_batch
FOV_TILE_POINTS = 256     # VFOV_BLOCK (csrc/velo_fov.hip): points one workgroup pass of the selection kernel takes
FOV_REG_POINTS = 4096     # VFOV_REG_POINTS: frames above this park their azimuths in scratch between the phases
IMU_FETCH_BATCH_MAX = 8192  # MML_IMU_FETCH_BATCH_MAX: intervals per call of mml_imu_fetch_batch / mml_imu_predict_batch
POSE_INGEST_MAX = 65535     # frames per call of mml_pose_ingest_batch / mml_pose_ingest_plan
# mml_imu_interval.status (csrc/imu_fetch.h)
IMU_FETCH_OK, IMU_FETCH_EMPTY, IMU_FETCH_NOT_REACHED, IMU_FETCH_TOO_OLD, IMU_FETCH_REVERSED, IMU_FETCH_NO_SAMPLE = 0, 1, 2, 3, 4, 5
UNION_OK, UNION_EMPTY, UNION_NOT_REACHED, UNION_NO_POINTS, UNION_OVERFLOW = 0, 1, 2, 3, 4   # mml_union_frame.status

LIVOX_DTYPE = np.dtype([("offset_time", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                        ("reflectivity", "u1"), ("tag", "u1"), ("line", "u1"), ("_pad", "u1")])


# mml_union_frame (C long: 8 bytes on the LP64 hosts ROCm runs on)
UNION_FRAME_DTYPE = np.dtype([("status", "<i4"), ("n_livox", "<i4"), ("begin", "<i8"), ("end", "<i8"), ("front_after", "<i8")])
# mml_imu_interval
IMU_INTERVAL_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("first", "<i8"), ("interpolated", "<i4"), ("_pad", "<i4"),
                               ("front_gyro_z", "<f8"), ("back_gyro_z", "<f8")])
# pcl::PointXYZINormal, 48 bytes: the record of mml_scan_download_pointxyzinormal / mml_feature_clouds_download_batch
POINTXYZINORMAL_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("data_pad", "<f4"), ("normal_x", "<f4"), ("normal_y", "<f4"),
                                  ("normal_z", "<f4"), ("normal_pad", "<f4"), ("intensity", "<f4"), ("curvature", "<f4"), ("pad0", "<f4"),
                                  ("pad1", "<f4")])
# raw points per block of the one-pass bucketing (MML_OP_BLK, csrc/mml_internal.h): a slot's storage is line-bucketed per block
ASSIGN_BLOCK_POINTS = 4096
# the clouds of union_cloud.msg:4-9, in the message's order: the cloud index of mml_feature_clouds_download_batch
FEATURE_CLOUD_NAMES = ("velo_corner", "velo_surface", "velo_combine", "livox_corner", "livox_surface", "livox_combine")
# mml_pose_ingest_row, and the values of its decision / reason fields (include/mmloam_hip.h)
POSE_INGEST_ROW_DTYPE = np.dtype([("decision", "<i4"), ("reason", "<i4"), ("fast_rotation", "<i4"), ("n_points", "<i4"), ("n_velo", "<i4"),
                                  ("_pad", "<i4")])
INGEST_VELO_ONLY, INGEST_MERGED, INGEST_DROPPED = 0, 1, 2
(INGEST_WHY_MERGED, INGEST_WHY_NO_IMU, INGEST_WHY_FIRST_FRAME, INGEST_WHY_VELO_ONLY_MODE, INGEST_WHY_FAST_ROTATION,
 INGEST_WHY_FEW_CORNERS) = range(6)
INGEST_WHY_FETCH = 16   # DROPPED: + the row's fetch status
# mml_time_offset_estimate_row, its status values, and the statuses of mml_time_offset_gate
TOFS_ROW_DTYPE = np.dtype([("status", "<i4"), ("n_kept", "<i4"), ("n_windows", "<i4"), ("best_window", "<i4"), ("lowest_error", "<f8"),
                           ("optim_start", "<u8"), ("time_offset", "<u8"), ("accepted", "<i4"), ("_pad", "<i4")])
TOFS_ROW_OK, TOFS_ROW_NO_VELO_IN_FOV = 0, 1
TOFS_GATE_OK, TOFS_GATE_EMPTY, TOFS_GATE_TOO_FEW_MESSAGES = 0, 1, 2
# mml_velo_fov_info
VELO_FOV_INFO_DTYPE = np.dtype([("start_ori", "<f4"), ("end_ori", "<f4"), ("half_index", "<i4"), ("n_kept", "<i4")])


def _signatures():
    """SIGNATURES: name -> (restype, [argtypes]) of every entry point, in the order and under the section titles of
    include/mmloam_hip.h.  One rule: any pointer parameter (handles included) is c_void_p, a scalar is its own ctypes type; a
    returned int is c_int, void None, const char* c_char_p, any other pointer c_void_p.  tests/test_abi_signatures.py holds the
    table against the header, declaration for declaration."""
    P, I, U, L, LL, U64, SZ, F, D, STR = (C.c_void_p, C.c_int, C.c_uint, C.c_long, C.c_longlong, C.c_uint64, C.c_size_t, C.c_float,
                                          C.c_double, C.c_char_p)
    return {
        # ---- (the header's head: configuration, contexts)
        "mml_config_default": (None, [P, I]), "mml_abi_version": (I, []), "mml_create": (I, [P, I, P]), "mml_destroy": (None, [P]),
        "mml_last_error": (STR, [P]), "mml_config_get": (I, [P, P]), "mml_synchronize": (I, [P]),
        # ---- input
        "mml_scan_upload": (I, [P, I, P, I, P, I]), "mml_scan_upload_batch": (I, [P, I, I, P, P, P, P]),
        "mml_scan_upload_pointcloud2": (I, [P, I, P, I, I, I, I, I, I, P, I]), "mml_scan_upload_wire": (I, [P, I, P, I, I, I, I, I, I, P, I]),
        "mml_scan_download_pointxyzinormal": (I, [P, I, P, I, P]), "mml_cloud_upload": (I, [P, I, P, I, I]),
        "mml_cloud_download_registered_batch": (I, [P, I, I, P, P, L, P]), "mml_cloud_download_registered": (I, [P, I, P, P, I, P]),
        "mml_world_map_create": (I, [P, I, F, L]), "mml_world_map_destroy": (I, [P]), "mml_world_map_reset": (I, [P, I]),
        "mml_world_map_add": (I, [P, I, I, P, P, U, P]), "mml_world_map_size": (I, [P, I, P]), "mml_world_map_download": (I, [P, I, P, P, L, P]),
        "mml_world_map_create_opts": (I, [P, I, F, L, U]), "mml_world_map_download_moments": (I, [P, I, P, L, P]),
        "mml_world_map_download_surfels": (I, [P, I, P, L, P]), "mml_feature_clouds_download_batch": (I, [P, I, I, P, L, P]),
        "mml_feature_clouds_download": (I, [P, I, P, I, P]),
        # ---- the aligner's time-offset search
        "mml_time_offset_search": (I, [P, P, I, P, P, I, I, I, P, P, I, P, P, P]),
        "mml_time_offset_search_batch": (I, [P, I, P, P, P, P, P, I, I, P, P, P, P, P, P]), "mml_time_offset_plan": (I, [I, P, P, I, I, I, P, P]),
        # ---- the aligner's Velodyne field-of-view selection: the input of the time-offset search
        "mml_velo_fov_select_batch": (I, [P, I, P, P, P, I, I, I, I, P, P, L, P, P]),
        "mml_velo_fov_select": (I, [P, P, I, I, I, I, I, P, P, I, P, P]),
        # ---- the aligner node's frame assembly: a Livox point stream cut into scan slots
        "mml_livox_stream_create": (I, [P, L, P]), "mml_livox_stream_destroy": (None, [P]), "mml_livox_stream_reset": (I, [P]),
        "mml_livox_stream_push": (I, [P, U64, P, I]), "mml_livox_stream_push_wire": (I, [P, U64, P, I]), "mml_livox_stream_state_get": (I, [P, P]),
        "mml_union_assemble": (I, [P, P, I, I, P, P, P, P, P]), "mml_union_plan": (I, [P, L, L, U64, I, P, I, P]),
        "mml_union_assemble_offset": (I, [P, P, I, I, P, I, P, P, P, P]), "mml_union_plan_offset": (I, [P, L, L, U64, I, P, I, P]),
        # ---- the aligner's time-offset estimation on the resident stream
        "mml_time_offset_estimate_stream": (I, [P, P, L, L, I, P, P, P, I, I, I, I, P, P, I, I, D, P, P, P, P]),
        "mml_time_offset_gate": (I, [I, P, U64, I, P, P]), "mml_scan_raw_download": (I, [P, I, P, I, P, I, P, P]),
        # ---- SURVEY section 8(f) rank 4 (the other part): the per-frame GICP extrinsic refresh
        "mml_gicp_align": (I, [P, P, I, P, I, P, P, P]), "mml_gicp_refresh": (I, [P, I, P, I, P, P]),
        "mml_gicp_align_batch": (I, [P, I, P, P, P, P, P, P, P]), "mml_gicp_refresh_batch": (I, [P, I, I, P, I, I, P, P]),
        "mml_gicp_align_opts": (I, [P, P, I, P, I, P, P, P, P]),
        # ---- the aligner node's start-up calibration
        "mml_cloud_crop_voxel": (I, [P, P, I, F, F, P, I, P, P]), "mml_aligner_calibrate": (I, [P, P, I, P, I, P, P, P, P]),
        # ---- a1..a8: feature extraction
        "mml_extract": (I, [P, I, I, P]), "mml_scan_info_get": (I, [P, I, P]), "mml_scan_download": (I, [P, I, P, P, P, P, I]),
        "mml_detect_line": (I, [P, P, I, P, P, P, P, P]),
        # ---- a9: RemoveLidarDistortion
        "mml_undistort": (I, [P, I, I, P, P]),
        # ---- a10: label split + pcl::VoxelGrid down-sample
        "mml_downsample": (I, [P, I, I]), "mml_features_download": (I, [P, I, I, P, I, P]), "mml_features_upload": (I, [P, I, I, P, I]),
        # ---- a13 map side: laserCloud{Corner,Surf}FromLocal
        "mml_map_set_local": (I, [P, I, P, I]),
        # ---- Estimator::MapIncrementLocal, on the device
        "mml_map_increment_local": (I, [P, I, P, P, P]), "mml_map_local_reset": (I, [P]), "mml_map_local_download": (I, [P, I, P, I, P]),
        # ---- SURVEY section 8(f) rank 2, global half: the MAP_MANAGER cube stores on the device
        "mml_map_global_append": (I, [P, I, P]), "mml_map_global_increment": (I, [P, P, P, P]),
        "mml_map_global_download": (I, [P, I, P, P, I, P, P]), "mml_map_global_reset": (I, [P]),
        # ---- a12: laserCloud{Corner,Surf}FromMap cube store
        "mml_map_set_global": (I, [P, I, P, P, I, P]),
        # ---- map banks: N further local maps per context, every scan slot matched against its own
        "mml_map_banks_create": (I, [P, I]), "mml_map_banks_destroy": (I, [P]), "mml_map_bank_set_local": (I, [P, I, I, P, I]),
        "mml_map_bank_reset": (I, [P, I]), "mml_map_bank_download": (I, [P, I, I, P, I, P]), "mml_slot_bind_bank": (I, [P, I, I, P]),
        "mml_slot_bank_get": (I, [P, I, I, P]), "mml_map_bank_increment": (I, [P, I, P, P, P, P, P]),
        "mml_map_bank_increment_segmented": (I, [P, I, P, P, P, P, P]), "mml_debug_bank_increment_budget": (I, [P, L]),
        "mml_map_bank_set_global": (I, [P, I, I, P, P, I, P]), "mml_map_bank_global_append": (I, [P, I, P, P, P]),
        "mml_map_bank_global_increment": (I, [P, I, P, P, P, P]), "mml_map_bank_global_increment_segmented": (I, [P, I, P, P, P, P]),
        "mml_map_bank_global_append_segmented": (I, [P, I, P, P, P]), "mml_debug_bank_global_increment_budget": (I, [P, L]),
        "mml_map_bank_global_download": (I, [P, I, I, P, P, I, P, P]), "mml_map_bank_global_reset": (I, [P, I]),
        "mml_knn5": (I, [P, I, P, I, F, P, P]),
        # ---- a11..a16: association + model fit
        "mml_associate": (I, [P, I, I, P, D, P]), "mml_factors_download": (I, [P, I, I, P, P, I, P]), "mml_factors_upload": (I, [P, I, I, P, I]),
        # ---- a17..a20: residual + Jacobian + normal equations
        "mml_linearize": (I, [P, I, P, P, D, D, P, P, P]), "mml_linearize_window": (I, [P, I, I, I, P, P, D, D, P]),
        "mml_solve": (I, [P, I, I, I, P, P, P, P, P]),
        # ---- a21: Estimator::Estimate, 1-frame mode
        "mml_estimate": (I, [P, I, I, P, P, P, I, I, P]),
        # ---- localisation in a surfel world map
        "mml_wm_assoc_opts_default": (None, [P, F]), "mml_wm_localize_opts_default": (None, [P, F]),
        "mml_world_map_export": (I, [P, I, P, P, P, P, L, P]), "mml_world_map_import": (I, [P, I, L, P, P, P, P]),
        "mml_world_map_associate": (I, [P, I, I, P, P, P, P]), "mml_world_map_localize": (I, [P, I, I, P, P, P, P, P, P]),
        # ---- relocalisation in a surfel world map: pose hypotheses scored on the device, a coarse-to-fine search
        "mml_wm_score_opts_default": (None, [P, F]), "mml_world_map_score": (I, [P, I, I, P, I, P, P, P]),
        "mml_wm_reloc_opts_default": (None, [P, F]), "mml_wm_pose_grid": (I, [P, D, D, D, D, D, D, P, L, P]),
        "mml_wm_body_pose": (I, [P, P, P, P]), "mml_wm_lidar_pose": (I, [P, P, P, P]), "mml_world_map_relocalize": (I, [P, I, I, P, P, P, P, P, P]),
        # ---- eviction: voxels leave the world map by box and by count, their rows handed back
        "mml_wm_index_box": (I, [F, P, P, P, P]), "mml_world_map_evict": (I, [P, I, P, U, P, L, P, P, P, P, P, P]),
        # ---- the benchmarked step
        "mml_step": (I, [P, I, I, P, P, P, D, I, P]),
        # ---- multi-GPU window solve (one frame per GPU)
        "mml_linearize_record": (I, [P, I, P, P, D, D, P]), "mml_window_solver_create": (P, [I, P]), "mml_window_solver_destroy": (None, [P]),
        "mml_window_solver_step": (I, [P, P, P]), "mml_window_solver_summary": (I, [P, P]),
        # ---- multi-GPU: RCCL inside the C-ABI
        "mml_comm_unique_id": (I, [P]), "mml_comm_init": (I, [P, I, I, P]), "mml_comm_destroy": (I, [P]), "mml_comm_info": (I, [P, P, P]),
        "mml_rccl_version": (I, [P]), "mml_window_solve_allgather": (I, [P, I, I, P, P, P, P, P, P]),
        "mml_comm_broadcast_features": (I, [P, I, I]), "mml_comm_broadcast_local_map": (I, [P, I]),
        # ---- loopback group: the N-rank path on ONE device
        "mml_comm_init_loopback": (I, [P, I]), "mml_window_solve_allgather_loopback": (I, [P, I, P, I, P, P, P, P, P]),
        "mml_comm_broadcast_features_loopback": (I, [P, I, I, I]), "mml_comm_broadcast_local_map_loopback": (I, [P, I, I]),
        # ---- verification hook: digests of the per-slot state
        "mml_slot_digest": (I, [P, I, I, P]),
        # ---- IMU factor, marginalization prior, full-window solve (host side)
        "mml_imu_preintegrate": (I, [P, I, P, P, P]), "mml_imu_factor": (I, [P, P, P, P, P, P, P, P]), "mml_fullwindow_create": (P, [I, P]),
        "mml_fullwindow_destroy": (None, [P]), "mml_fullwindow_set_imu": (I, [P, I, P, P]), "mml_fullwindow_set_prior": (I, [P, P]),
        "mml_fullwindow_step": (I, [P, P, P]), "mml_fullwindow_summary": (I, [P, P]),
        "mml_fullwindow_normal_equations": (I, [P, P, P, P, P, P]), "mml_fullwindow_marginalize": (I, [P, P, P, P]),
        # ---- the LIO initialisation that opens full-window mode, and the batched calls
        "mml_imu_gyro_integrate": (I, [P, I, P]), "mml_imu_init_factor": (I, [P, P, P, P, P, P, P, P, P, P, P]),
        "mml_lio_initialize": (I, [I, P, P, P, P, P, P, P, P, P, P, P, P]), "mml_fullwindow_solve": (I, [P, P, I, P, P, P, P]),
        "mml_fullwindow_solve_batch": (I, [P, I, P, P, P, P, P, P, P]), "mml_fullwindow_marginalize_batch": (I, [P, I, P, P, P, P, P]),
        "mml_imu_preintegrate_batch": (I, [P, I, P, P, P, P, P]), "mml_lio_initialize_batch": (I, [P, I, P, P, P, P, P, P, P, P, P, P, P, P, P]),
        # ---- the pose node's IMU queue: a device-resident message store cut and pre-integrated per frame interval
        "mml_imu_stream_create": (I, [P, L, P]), "mml_imu_stream_destroy": (None, [P]), "mml_imu_stream_reset": (I, [P]),
        "mml_imu_stream_push": (I, [P, P, I]), "mml_imu_stream_drop_before": (I, [P, D, L]), "mml_imu_stream_state_get": (I, [P, P]),
        "mml_imu_fetch_batch": (I, [P, P, I, P, P, P, P, P, P, P, L, P, P]), "mml_imu_fetch_host": (I, [P, L, I, P, P, P, P, P, P, P, L, P, P]),
        "mml_imu_predict_batch": (I, [P, I, P, P, P, P, P, P, P, P, P]),
        # ---- the pose node's way in: `count` union_cloud messages into scan slots in one call
        "mml_pose_ingest_opts_default": (None, [P]), "mml_pose_ingest_plan": (I, [I, P, P, P, P]),
        "mml_pose_ingest_batch": (I, [P, I, I, P, P, P, P, P]),
        # ---- the feature node's way in: `count` union_cloud messages in wire form into scan slots in one call
        "mml_scan_upload_wire_batch": (I, [P, I, I, P, P, P, I, I, I, I, I, P, P, P, I]),
        "mml_scan_upload_wire_plan": (I, [I, P, P, I, I, I, I, I, P, P, I, I, I, P, P]),
        "mml_wire_decode_host": (I, [I, P, P, P, I, I, I, I, I, P, P, P, I, P, P]),
        # ---- (the header's tail: measurement and test hooks)
        "mml_set_lanes": (I, [P, I]), "mml_profile_enable": (I, [P, I]), "mml_profile_reset": (I, [P]), "mml_profile_get": (I, [P, P]),
        "mml_extract_queue_counts": (I, [P, I, P, P]), "mml_libm_f32": (I, [P, P, P, L, P, P]), "mml_model_fit5": (I, [P, I, P, L, P]),
        "mml_marginalize_dense": (I, [P, L, P, P, P, P]), "mml_debug_tr_replay": (I, [P, I, I, I, P, P, P, P, P, P]),
        "mml_debug_fw_replay": (I, [P, I, I, P, P, P, P, LL, P, P, P]), "mml_debug_gicp": (I, [P, I, P]),
        "mml_associate_far_count": (I, [P, P]), "mml_device_info": (I, [P, P, I, P, P]), "mml_copy_bandwidth": (I, [P, SZ, I, P]),
        "mml_issue_rate": (I, [P, I, I, P]),
        # ---- not in the public header (NOT_IN_HEADER): exported by csrc/capi.hip for tools/phases.py
        "mml_debug_phase_clocks": (I, [P, P, I, I]),
    }


SIGNATURES = _signatures()
NOT_IN_HEADER = ("mml_debug_phase_clocks",)
# the world map's entry points by the change that brought them (tests/test_world_map_*.py): views onto SIGNATURES
WORLD_MAP_ARGTYPES, WORLD_MAP_SURFEL_ARGTYPES, WORLD_MAP_LOCALIZE_ARGTYPES, WORLD_MAP_SCORE_ARGTYPES = (
    {n: SIGNATURES[n][1] for n in names} for names in (
        ("mml_world_map_create", "mml_world_map_destroy", "mml_world_map_reset", "mml_world_map_add", "mml_world_map_size",
         "mml_world_map_download"),
        ("mml_world_map_create_opts", "mml_world_map_download_moments", "mml_world_map_download_surfels"),
        ("mml_world_map_export", "mml_world_map_import", "mml_world_map_associate", "mml_world_map_localize"),
        ("mml_world_map_score", "mml_wm_pose_grid", "mml_wm_body_pose", "mml_wm_lidar_pose", "mml_world_map_relocalize")))


class MmlError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mmloam_hip error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("max_scans", C.c_int), ("max_velo_points", C.c_int), ("max_livox_points", C.c_int),
                ("n_rings", C.c_int), ("pitch0_deg", C.c_float), ("pitch_step_deg", C.c_float),
                ("n_livox_lines", C.c_int), ("near_th", C.c_float), ("far_th", C.c_float),
                ("leaf_corner", C.c_float), ("leaf_surf", C.c_float), ("cell_corner", C.c_float),
                ("cell_surf", C.c_float), ("max_features", C.c_int), ("max_map_points", C.c_int)]


class ScanInfo(C.Structure):
    _fields_ = [("n_points", C.c_int), ("n_velo", C.c_int), ("velo_corner_num", C.c_int), ("velo_surf_num", C.c_int),
                ("livox_corner_num", C.c_int), ("livox_surf_num", C.c_int), ("fused_corner_num", C.c_int),
                ("fused_surf_num", C.c_int)]


class AssocStats(C.Structure):
    _fields_ = [("n_line", C.c_int), ("n_plane", C.c_int), ("n_line_used", C.c_int), ("n_plane_used", C.c_int),
                ("normal_gram", C.c_double * 9), ("min_singular", C.c_double), ("is_degenerate", C.c_int)]


class SolveOpts(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int), ("fixed_iterations", C.c_int), ("huber_delta", C.c_double),
                ("plan_weight_tan", C.c_double)]


class SolveSummary(C.Structure):
    _fields_ = [("iterations", C.c_int), ("successful", C.c_int), ("initial_cost", C.c_double),
                ("final_cost", C.c_double), ("termination", C.c_int)]


class EstimateInfo(C.Structure):
    _fields_ = [("outer_iterations", C.c_int), ("is_degenerate", C.c_int), ("n_corner_feat", C.c_int),
                ("n_surf_feat", C.c_int)]


class WindowTiming(C.Structure):
    _fields_ = [("evaluations", C.c_int), ("rounds", C.c_int), ("exchanges", C.c_int), ("device_ms", C.c_double)]


COMM_ID_BYTES = 128


class LoopbackGroup:
    """N contexts of this process on one device as the ranks 0 .. N-1 of a communicator whose collectives are device copies
    (mml_comm_*_loopback): the N-rank path of the C-ABI on a single GPU.  Every call drives all ranks."""

    def __init__(self, contexts):
        self.ctxs = list(contexts)
        self.n = len(self.ctxs)
        self._arr = (C.c_void_p * self.n)(*[c._h for c in self.ctxs])
        self._ck(lib().mml_comm_init_loopback(self._arr, self.n), "mml_comm_init_loopback")

    def _ck(self, rc, what):
        if rc != 0:
            errs = [lib().mml_last_error(c._h).decode() for c in self.ctxs]
            raise MmlError(rc, what + ": " + " | ".join(e for e in errs if e))

    def window_solve(self, first_slots, n_local, x_window, T_bl, max_iters=10, fixed=False, huber=0.0, w_tan=3e-4):
        """Returns (n_ranks x W x 6 poses as every rank holds them, per-rank summaries)."""
        W = self.n * n_local
        x = _f64(x_window).reshape(W, 6).copy()
        out = np.zeros((self.n, W, 6))
        fs = np.ascontiguousarray(first_slots, dtype=np.int32)
        opts = SolveOpts(max_iters, 1 if fixed else 0, huber, w_tan)
        summ = (SolveSummary * self.n)()
        self._ck(lib().mml_window_solve_allgather_loopback(self._arr, self.n, _p(fs), n_local, _p(_f64(T_bl).reshape(16)), C.byref(opts), _p(x),
                                                           _p(out), summ), "mml_window_solve_allgather_loopback")
        return out, list(summ)

    def broadcast_features(self, slot, root):
        self._ck(lib().mml_comm_broadcast_features_loopback(self._arr, self.n, slot, root), "mml_comm_broadcast_features_loopback")

    def broadcast_local_map(self, root):
        self._ck(lib().mml_comm_broadcast_local_map_loopback(self._arr, self.n, root), "mml_comm_broadcast_local_map_loopback")


def comm_unique_id():
    """ncclGetUniqueId through the C-ABI: called by one rank, handed to mml_comm_init of every rank."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = lib().mml_comm_unique_id(buf)
    if rc != MML_OK:
        raise MmlError(rc, "mml_comm_unique_id")
    return bytes(buf)


class GicpInfo(C.Structure):
    _fields_ = [("outer_iterations", C.c_int), ("objective_evaluations", C.c_int), ("objective", C.c_double),
                ("n_source", C.c_int), ("n_target", C.c_int)]


class GicpOpts(C.Structure):
    """mml_gicp_opts: setMaximumIterations, setTransformationEpsilon, setMaxCorrespondenceDistance (<= 0: no gate)."""
    _fields_ = [("max_iterations", C.c_int), ("transformation_epsilon", C.c_double), ("max_correspondence_distance", C.c_double)]


GICP_DBG_COV, GICP_DBG_CORR, GICP_DBG_EVAL, GICP_DBG_INTERP, GICP_DBG_QUAD, GICP_DBG_STATE, GICP_DBG_ROUND = range(7)


class GicpDebug(C.Structure):
    """mml_gicp_debug: the inputs and outputs of mml_debug_gicp."""
    _fields_ = [(n, C.c_void_p) for n in ("src", "tgt", "cov_src", "cov_tgt", "T", "corr", "maha", "x", "out_d", "out_i", "out_f")] + [
        ("gate2", C.c_double), ("transformation_epsilon", C.c_double), ("n_src", C.c_int), ("n_tgt", C.c_int), ("k", C.c_int),
        ("grad", C.c_int), ("max_iterations", C.c_int), ("_pad", C.c_int)]


class CalibInfo(C.Structure):
    _fields_ = [("n_hori_in", C.c_int), ("n_velo_in", C.c_int), ("n_hori_ds", C.c_int), ("n_velo_ds", C.c_int),
                ("hori_unfiltered", C.c_int), ("velo_unfiltered", C.c_int), ("gicp", GicpInfo)]


class PoseIngestOpts(C.Structure):
    _fields_ = [("hori_rotate_th", C.c_double), ("velo_rotate_th", C.c_double), ("velo_only_mode", C.c_int), ("first_frame", C.c_int)]


class Profile(C.Structure):
    _fields_ = [("n_stages", C.c_int), ("name", C.c_char_p * MAX_STAGES), ("total_ms", C.c_double * MAX_STAGES),
                ("launches", C.c_long * MAX_STAGES)]


class WorldMapInfo(C.Structure):
    """mml_world_map_info: what one mml_world_map_add call did."""
    _fields_ = [(k, C.c_long) for k in ("n_points", "n_kept", "n_nonfinite", "n_out_of_range", "n_masked", "n_new_voxels",
                                        "n_voxels_total")]


MML_WM_SURFELS = 1   # the flag of mml_world_map_create_opts (include/mmloam_hip.h, "Surfel maps")


# localisation in a surfel map (include/mmloam_hip.h, "localisation in a surfel world map")
class WmAssocOpts(C.Structure):
    """mml_wm_assoc_opts"""
    _fields_ = [("neighbourhood", C.c_int), ("min_points", C.c_int), ("min_planarity", C.c_float), ("max_plane_dist", C.c_double)]


class WmLocalizeOpts(C.Structure):
    """mml_wm_localize_opts"""
    _fields_ = [("assoc", WmAssocOpts), ("max_plane_dist_by_outer", C.c_double * 3), ("max_outer", C.c_int), ("inner_iters", C.c_int)]


def wm_assoc_opts(leaf, **over):
    """mml_wm_assoc_opts_default(leaf) with fields replaced"""
    o = WmAssocOpts()
    lib().mml_wm_assoc_opts_default(C.byref(o), leaf)
    for k, v in over.items():
        setattr(o, k, v)
    return o


def wm_localize_opts(leaf, **over):
    """mml_wm_localize_opts_default(leaf) with fields replaced; max_plane_dist_by_outer: three values; assoc: a WmAssocOpts"""
    o = WmLocalizeOpts()
    lib().mml_wm_localize_opts_default(C.byref(o), leaf)
    for k, v in over.items():
        setattr(o, k, (C.c_double * 3)(*v) if k == "max_plane_dist_by_outer" else v)
    return o


# ... and relocalisation in it (include/mmloam_hip.h, "relocalisation in a surfel world map")
class WmScore(C.Structure):
    """mml_wm_score"""
    _fields_ = [("score_q", C.c_ulonglong), ("n_match", C.c_int), ("n_scored", C.c_int)]


WM_SCORE_DT = np.dtype([("score_q", np.uint64), ("n_match", np.int32), ("n_scored", np.int32)])


class WmScoreOpts(C.Structure):
    """mml_wm_score_opts"""
    _fields_ = [("assoc", WmAssocOpts), ("stride", C.c_int)]


class WmRelocOpts(C.Structure):
    """mml_wm_reloc_opts"""
    _fields_ = [("half_xy", C.c_double), ("step_xy", C.c_double), ("half_z", C.c_double), ("step_z", C.c_double), ("half_yaw", C.c_double),
                ("step_yaw", C.c_double), ("levels", C.c_int), ("refine", C.c_int), ("keep", C.c_int), ("score", WmScoreOpts),
                ("localize", WmLocalizeOpts)]


class WmRelocInfo(C.Structure):
    """mml_wm_reloc_info"""
    _fields_ = [("best", WmScore), ("second", WmScore), ("final", WmScore), ("n_hyp_scored", C.c_long), ("T_start", C.c_double * 16),
                ("est", EstimateInfo)]


# ... and eviction from it (include/mmloam_hip.h, "eviction")
WM_EVICT_OUTSIDE, WM_EVICT_INSIDE, WM_EVICT_NOBOX = 0, 1, 2   # mml_wm_evict_rule.mode
MML_WM_EVICT_DRY = 1                                          # the flag of mml_world_map_evict


class WmEvictRule(C.Structure):
    """mml_wm_evict_rule"""
    _fields_ = [("map", C.c_int), ("mode", C.c_int), ("lo", C.c_int * 3), ("hi", C.c_int * 3), ("min_count", C.c_int)]


class WmEvictInfo(C.Structure):
    """mml_wm_evict_info"""
    _fields_ = [(k, C.c_long) for k in ("n_before", "n_evicted", "n_kept", "first_row")]


def wm_evict_rule(map, mode=WM_EVICT_NOBOX, lo=(0, 0, 0), hi=(0, 0, 0), min_count=0):
    """One mml_wm_evict_rule: the voxels of `map` outside / inside the index box [lo, hi) go (mode), and those below min_count"""
    return WmEvictRule(int(map), int(mode), (C.c_int * 3)(*[int(v) for v in lo]), (C.c_int * 3)(*[int(v) for v in hi]), int(min_count))


def wm_index_box(leaf, lo_xyz, hi_xyz):
    """mml_wm_index_box: the index box (lo, hi), two (3,) int32, of the metric box [lo_xyz, hi_xyz] in a map of leaf size `leaf`"""
    lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    rc = lib().mml_wm_index_box(float(leaf), _p(_f32(lo_xyz).reshape(3)), _p(_f32(hi_xyz).reshape(3)), _p(lo), _p(hi))
    if rc != MML_OK:
        raise MmlError(rc, "mml_wm_index_box: refused (a coordinate or the leaf not finite, leaf <= 0)")
    return lo, hi


def wm_score_opts(leaf, **over):
    """mml_wm_score_opts_default(leaf) with fields replaced; the fields of `assoc` may be given directly (max_plane_dist=...)"""
    o = WmScoreOpts()
    lib().mml_wm_score_opts_default(C.byref(o), leaf)
    for k, v in over.items():
        setattr(o.assoc if k in ("neighbourhood", "min_points", "min_planarity", "max_plane_dist") else o, k, v)
    return o


def wm_reloc_opts(leaf, **over):
    """mml_wm_reloc_opts_default(leaf) with fields replaced; score: a WmScoreOpts, localize: a WmLocalizeOpts"""
    o = WmRelocOpts()
    lib().mml_wm_reloc_opts_default(C.byref(o), leaf)
    for k, v in over.items():
        setattr(o, k, v)
    return o


def wm_pose_grid(seed, half_xy, step_xy, half_z=0.0, step_z=1.0, half_yaw=0.0, step_yaw=1.0):
    """mml_wm_pose_grid: the (H, 4, 4) hypotheses of the grid around the pose `seed`, index ((iyaw nz + iz) ny + iy) nx + ix"""
    seed = _f64(seed).reshape(16)
    n = C.c_long(0)
    a = [float(v) for v in (half_xy, step_xy, half_z, step_z, half_yaw, step_yaw)]
    rc = lib().mml_wm_pose_grid(_p(seed), *a, None, 0, C.byref(n))
    if rc != MML_OK:
        raise MmlError(rc, "mml_wm_pose_grid: refused (a value not finite, a negative half, half_yaw > pi, a step <= 0, too many cells)")
    out = np.zeros((n.value, 4, 4))
    rc = lib().mml_wm_pose_grid(_p(seed), *a, _p(out), n.value, C.byref(n))
    if rc != MML_OK:
        raise MmlError(rc, "mml_wm_pose_grid")
    return out


def wm_body_pose(T_wl, exTlb):
    """mml_wm_body_pose: P (3), Q (4, x y z w) of the body from the lidar pose T_wl and exTlb"""
    P, Q = np.zeros(3), np.zeros(4)
    rc = lib().mml_wm_body_pose(_p(_f64(T_wl).reshape(16)), _p(_f64(exTlb).reshape(16)), _p(P), _p(Q))
    if rc != MML_OK:
        raise MmlError(rc, "mml_wm_body_pose")
    return P, Q


def wm_lidar_pose(P, Q, exTlb):
    """mml_wm_lidar_pose: the (4, 4) lidar pose T_wl = [Q, P] inverse(exTlb), as the pose calls compose it"""
    T = np.zeros((4, 4))
    rc = lib().mml_wm_lidar_pose(_p(_f64(P).reshape(3)), _p(_f64(Q).reshape(4)), _p(_f64(exTlb).reshape(16)), _p(T))
    if rc != MML_OK:
        raise MmlError(rc, "mml_wm_lidar_pose")
    return T


def build(force=False):
    """Compile csrc/*.hip for gfx950 into libmmloam_hip.so (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "-s", "clean"])
    subprocess.check_call(["make", "-C", csrc, "-s", "-j8"])
    return LIB_PATH


_lib = None


def rccl_libraries():
    """ONE RCCL per process is what a multi-rank run wants.  libmmloam_hip.so needs `librccl.so.1` / `libamdhip64.so.7` (the
    ROCm copies, by its RUNPATH); a PyTorch wheel ships its own `torch/lib/librccl.so` and `libamdhip64.so` with the same
    SONAMEs.  The dynamic loader identifies a library by SONAME and by file: when torch is imported FIRST, our NEEDED entries
    resolve to its copies and the process holds one HIP runtime and one RCCL; the other way round torch's `librccl.so` request
    matches neither the name nor the file of the ROCm copy and a second runtime and a second RCCL would be mapped.  lib()
    therefore maps torch's copies itself before loading the library (_share_torch_runtime), so the order of the imports no
    longer matters; Context.comm_init still refuses to build a communicator of more than one rank when two copies are mapped.
    Returns the paths of every librccl in /proc/self/maps and the version behind the C-ABI's collectives."""
    v = C.c_int(0)
    lib().mml_rccl_version(C.byref(v))
    paths = []
    try:
        for line in open("/proc/self/maps"):
            f = line.split()
            # the library itself, not what it loads: RCCL dlopens net plugins (librccl-net.so, librccl-net-ofi.so ...) during init
            if len(f) >= 6 and f[5] not in paths and re.fullmatch(r"librccl\.so(\.\d+)*", os.path.basename(f[5])):
                paths.append(f[5])
    except OSError:
        pass
    return dict(loaded=paths, version=v.value)


def _share_torch_runtime():
    """Import-order independence of "one HIP runtime, one RCCL per process" (see rccl_libraries): when a PyTorch wheel with its
    own `libamdhip64.so` / `librccl.so` is installed, map THOSE files (by path, without importing torch) before
    libmmloam_hip.so is loaded.  Their SONAMEs are `libamdhip64.so.7` / `librccl.so.1`, so our NEEDED entries then bind to them,
    and a later `import torch` finds its own files already mapped -- the state "torch imported first" used to give, whichever
    comes first.  Without torch (a C++ host, a torch-free Python) nothing is preloaded and the ROCm copies are used.
    $MML_NO_TORCH_RUNTIME=1 switches the preload off."""
    if os.environ.get("MML_NO_TORCH_RUNTIME") == "1":
        return []
    done = []
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return done
        tl = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        for name in ("libamdhip64.so", "librccl.so"):
            path = os.path.join(tl, name)
            if os.path.exists(path):
                # RTLD_LOCAL: the loader's SONAME / file matching does not depend on symbol visibility, and RCCL's symbols put
                # into the global scope ahead of torch's own libraries end in a double free at process exit (measured)
                C.CDLL(path, mode=C.RTLD_LOCAL)
                done.append(path)
    except OSError:
        pass   # an unloadable wheel copy: fall back to the ROCm copies (rccl_libraries() still reports what is mapped)
    return done


def _bind(L):
    """SIGNATURES onto the entry points of the loaded library L.  A name L lacks is skipped: an A/B build of an older commit
    through $MML_LIB_PATH has not got the newest ones, and still loads."""
    for name, (restype, argtypes) in SIGNATURES.items():
        f = getattr(L, name, None)
        if f is not None:
            f.restype, f.argtypes = restype, argtypes


def lib():
    """Load libmmloam_hip.so; fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MmlError(MML_ERR_STATE, "libmmloam_hip.so is missing: run __graft_entry__.build() "
                                          "(or make -C multi-modal-loam_amd/csrc); there is no CPU fallback")
        _share_torch_runtime()
        L = C.CDLL(LIB_PATH)
        _bind(L)
        _lib = L
    return _lib


def cube_index(xyz, cen=(10, 5, 10)):
    """Cube of every map-frame point, MAP_MANAGER::FindUsedCornerMap / FindUsedSurfMap (Map_Manager.cpp:583-629):
    ToIndex(i, j, k) = i + 21 j + 441 k over the 21 x 21 x 11 grid of 50 m cubes, 5000 for a point outside it.
    cen = laserCloudCen{Width,Height,Depth}_last.  Used to tag a global map for Context.map_set_global."""
    p = _f32(xyz).reshape(-1, 3).astype(np.float64)
    q = (p + 25.0) / 50.0
    with np.errstate(invalid="ignore"):
        c = np.where(np.isfinite(q), np.trunc(q), -1.0e6).astype(np.int64)
    c -= (p + 25.0 < 0)
    ci, cj, ck = c[:, 0] + cen[2], c[:, 1] + cen[0], c[:, 2] + cen[1]
    ok = (ci >= 0) & (ci < 21) & (cj >= 0) & (cj < 21) & (ck >= 0) & (ck < 11)
    return np.where(ok, ci + 21 * cj + 441 * ck, 5000).astype(np.int32)


def default_config(max_scans=1, **over):
    cfg = Config()
    lib().mml_config_default(C.byref(cfg), max_scans)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def registered_poses(count, T_wl):
    """The pose argument of mml_cloud_download_registered_batch: (count, 16) float64 from count 4 x 4 matrices -- (count, 4, 4)
    or (count, 16); one (4, 4) or (16,) pose is accepted when count == 1.  ValueError for anything else."""
    count = int(count)
    if count < 1:
        raise ValueError("count must be at least 1, not %d" % count)
    T = np.asarray(T_wl, dtype=np.float64)
    if T.shape in ((4, 4), (16,)):
        if count != 1:
            raise ValueError("one pose given for %d slots: T_wl must hold one 4 x 4 matrix per slot" % count)
    elif T.ndim < 2 or T.shape[1:] not in ((4, 4), (16,)):
        raise ValueError("T_wl must be (count, 4, 4) or (count, 16), not %s" % (T.shape,))
    elif T.shape[0] != count:
        raise ValueError("T_wl holds %d poses for %d slots" % (T.shape[0], count))
    return np.ascontiguousarray(T.reshape(count, 16))


def gicp_pack_pairs(pairs, T0=None):
    """The arguments of mml_gicp_align_batch for a ragged list of (src, tgt) clouds: (src n x 3 float32, src_offsets int32[n + 1],
    tgt, tgt_offsets, T float32[n, 4, 4]).  T0: None (identities), one 4 x 4 matrix for every problem, or n of them."""
    n = len(pairs)
    srcs = [_f32(s).reshape(-1, 3) for s, _ in pairs]
    tgts = [_f32(t).reshape(-1, 3) for _, t in pairs]
    so = np.zeros(n + 1, np.int32)
    to = np.zeros(n + 1, np.int32)
    so[1:] = np.cumsum([len(s) for s in srcs])
    to[1:] = np.cumsum([len(t) for t in tgts])
    src = np.ascontiguousarray(np.concatenate(srcs + [np.zeros((0, 3), np.float32)]))
    tgt = np.ascontiguousarray(np.concatenate(tgts + [np.zeros((0, 3), np.float32)]))
    if T0 is None:
        T = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    else:
        T0 = np.asarray(T0, np.float32)
        T = np.tile(T0, (n, 1, 1)) if T0.size == 16 else T0.reshape(n, 4, 4).copy()
    return src, so, tgt, to, np.ascontiguousarray(T)


def time_offset_pack(velo_list, livox_list, tfs=None):
    """The arguments of mml_time_offset_search_batch for ragged lists of clouds: (velo n x 3 float32, velo_offsets int32[n + 1],
    livox, livox_offsets, tf float32[n, 16] or None).  tfs: None (no problem is transformed), one 4 x 4 matrix for every problem,
    or n of them."""
    if len(velo_list) != len(livox_list):
        raise ValueError("%d Velodyne clouds for %d Livox clouds" % (len(velo_list), len(livox_list)))
    n = len(velo_list)
    vs = [_f32(v).reshape(-1, 3) for v in velo_list]
    ls = [_f32(l).reshape(-1, 3) for l in livox_list]
    vo = np.zeros(n + 1, np.int32)
    lo = np.zeros(n + 1, np.int32)
    vo[1:] = np.cumsum([len(v) for v in vs])
    lo[1:] = np.cumsum([len(l) for l in ls])
    velo = np.ascontiguousarray(np.concatenate(vs + [np.zeros((0, 3), np.float32)]))
    livox = np.ascontiguousarray(np.concatenate(ls + [np.zeros((0, 3), np.float32)]))
    tf = None
    if tfs is not None:
        t = np.asarray(tfs, np.float32)
        tf = np.ascontiguousarray(np.tile(t.reshape(1, 16), (n, 1)) if t.size == 16 else t.reshape(n, 16).copy())
    return velo, vo, livox, lo, tf


def time_offset_plan(velo_offsets, livox_offsets, search_resolution=30, sliced_points=12000, max_map_points=-1):
    """mml_time_offset_plan: the host-only checks of mml_time_offset_search_batch (no context, no device).  Returns
    (code, bad_problem, n_windows int32[n]); n_windows is filled only when code == MML_OK.  max_map_points < 0: no capacity check."""
    vo = np.ascontiguousarray(velo_offsets, dtype=np.int32)
    lo = np.ascontiguousarray(livox_offsets, dtype=np.int32)
    if len(vo) != len(lo):
        raise ValueError("the two offset arrays must have the same length (n + 1)")
    n = len(vo) - 1
    nwin = np.zeros(max(n, 1), np.int32)
    bad = C.c_int(-1)
    rc = lib().mml_time_offset_plan(n, _p(vo), _p(lo), search_resolution, sliced_points, max_map_points, _p(nwin), C.byref(bad))
    return rc, bad.value, nwin[:max(n, 0)]


def time_offset_gate(velo_stamps, hori_stamp, n_hori_msgs):
    """mml_time_offset_gate (host only): which queued Velodyne frame estimate_timeoffset runs on, the loop of
    unionLidarsAligner.cpp:1026-1043.  velo_stamps: the queued frames' header stamps in ns, oldest first; hori_stamp: the newest
    Livox message's header stamp; n_hori_msgs: queued Livox messages.  Returns (selected, status): the frame's index and
    TOFS_GATE_OK, or -1 and TOFS_GATE_EMPTY (every frame popped) / TOFS_GATE_TOO_FEW_MESSAGES (fewer than 8 messages)."""
    vs = np.ascontiguousarray(velo_stamps, dtype=np.uint64)
    sel, st = C.c_int(-7), C.c_int(-7)
    rc = lib().mml_time_offset_gate(len(vs), _p(vs) if len(vs) else None, int(hori_stamp), n_hori_msgs, C.byref(sel), C.byref(st))
    if rc != MML_OK:
        raise MmlError(rc, "mml_time_offset_gate")
    return sel.value, st.value


def velo_fov_pack(frames):
    """The input arguments of mml_velo_fov_select_batch for a list of frames, each an (n_i, k) float32 array with k >= 3 whose
    columns start x, y, z: (data uint8, byte_offsets int64[n], n_points int32[n], point_step).  All frames must share k."""
    fs = [_f32(f) for f in frames]
    fs = [f.reshape(-1, f.shape[-1] if f.ndim > 1 else 3) for f in fs]
    ks = {f.shape[1] for f in fs}
    if len(ks) > 1 or (ks and min(ks) < 3):
        raise ValueError("frames must share one row width of at least 3 floats (x, y, z, ...), not %s" % sorted(ks))
    k = ks.pop() if ks else 4
    n_points = np.array([len(f) for f in fs], np.int32)
    byte_offsets = np.zeros(len(fs), np.int64)
    if len(fs):
        byte_offsets[1:] = np.cumsum(n_points[:-1].astype(np.int64)) * 4 * k
    data = np.ascontiguousarray(np.concatenate(fs + [np.zeros((0, k), np.float32)])).reshape(-1).view(np.uint8)
    return data, byte_offsets, n_points, 4 * k


def velo_fov_select_raw(data, byte_offsets, n_points, point_step, off_x=0, off_y=4, off_z=8, ctx=None):
    """mml_velo_fov_select_batch on PointCloud2-style payloads: frame i is n_points[i] records of point_step bytes at
    data[byte_offsets[i]:] with float32 fields at off_x / off_y / off_z.  The sizing call and the filling call.  Returns a dict:
    xyzt (total, 4) float32 = x, y, z, relTime of the kept points; xyz (total, 3), the velo_xyz of time_offset_search_batch;
    n_kept int32[n]; offsets int32[n + 1], its velo_offsets; info VELO_FOV_INFO_DTYPE[n].  ctx None: the host routine."""
    raw = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    bo = np.ascontiguousarray(byte_offsets, dtype=np.int64)   # (C long: 8 bytes on the LP64 hosts ROCm runs on)
    npts = np.ascontiguousarray(n_points, dtype=np.int32)
    if len(bo) != len(npts):
        raise ValueError("%d byte offsets for %d point counts" % (len(bo), len(npts)))
    n = len(npts)
    if n and point_step > 0 and int((bo + npts.astype(np.int64) * point_step).max()) > len(raw) and bo.min() >= 0 and npts.min() >= 0:
        raise ValueError("a frame ends beyond the %d bytes of data" % len(raw))
    h = ctx._h if ctx is not None else None

    def call(xyzt, xyz, cap, kept, info):
        rc = lib().mml_velo_fov_select_batch(h, n, _p(raw) if len(raw) else None, _p(bo), _p(npts), point_step, off_x, off_y, off_z, _p(xyzt),
                                             _p(xyz), cap, _p(kept), _p(info))
        if ctx is not None:
            ctx._ck(rc)
        elif rc != MML_OK:
            raise MmlError(rc, "mml_velo_fov_select_batch")

    kept = np.zeros(max(n, 1), np.int32)
    info = np.zeros(max(n, 1), VELO_FOV_INFO_DTYPE)
    call(None, None, 0, kept, info)
    total = int(kept[:n].sum())
    xyzt = np.zeros((max(total, 1), 4), np.float32)
    xyz = np.zeros((max(total, 1), 3), np.float32)
    if total:
        call(xyzt, xyz, total, kept, info)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum(kept[:n])
    return {"xyzt": xyzt[:total], "xyz": xyz[:total], "n_kept": kept[:n], "offsets": offsets, "info": info[:n]}


def velo_fov_select(frames, ctx=None):
    """velo_cloud_handler's FOV selection (unionLidarsAligner.cpp:437-490) for a list of Velodyne frames, each (n_i, k >= 3)
    float32 rows x, y, z, ...: velo_fov_select_raw on their packed bytes.  ctx None: the host routine (no device needed); a
    Context: the device kernels, equal to it to the byte."""
    data, bo, npts, step = velo_fov_pack(frames)
    return velo_fov_select_raw(data, bo, npts, step, 0, 4, 8, ctx=ctx)


def union_plan(S, front, tail, hs, stamps, max_livox_points):
    """mml_union_plan: the frame rows mml_union_assemble returns, on the host alone (no context, no device), for a stream whose
    stamps are the array S indexed absolutely (S[front] .. S[tail - 1] are read).  stamps: count + 1 frame boundaries in absolute
    nanoseconds.  Returns (code, rows UNION_FRAME_DTYPE[count]); the rows are filled only when code == MML_OK."""
    Sa = np.ascontiguousarray(S, dtype=np.uint64)
    st = np.ascontiguousarray(stamps, dtype=np.uint64)
    count = len(st) - 1
    if tail > len(Sa):
        raise ValueError("tail = %d lies beyond the %d stamps given" % (tail, len(Sa)))
    rows = np.zeros(max(count, 1), UNION_FRAME_DTYPE)
    rc = lib().mml_union_plan(_p(Sa) if len(Sa) else None, front, tail, int(hs), count, _p(st), max_livox_points, _p(rows))
    return rc, rows[:max(count, 0)]


def union_plan_offset(S, front, tail, hs, starts, sliced_points):
    """mml_union_plan_offset: the frame rows mml_union_assemble_offset returns, on the host alone, for the stamp array S (as
    union_plan reads it).  starts: one stamp per frame in absolute nanoseconds; each frame takes up to sliced_points points from the
    first one at or after its stamp.  Returns (code, rows UNION_FRAME_DTYPE[count]); the rows are filled only when code == MML_OK."""
    Sa = np.ascontiguousarray(S, dtype=np.uint64)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    count = len(st)
    if tail > len(Sa):
        raise ValueError("tail = %d lies beyond the %d stamps given" % (tail, len(Sa)))
    rows = np.zeros(max(count, 1), UNION_FRAME_DTYPE)
    rc = lib().mml_union_plan_offset(_p(Sa) if len(Sa) else None, front, tail, int(hs), count, _p(st) if count else None, sliced_points, _p(rows))
    return rc, rows[:count]


class LivoxStreamState(C.Structure):
    _fields_ = [("start_stamp", C.c_uint64), ("front", C.c_long), ("tail", C.c_long), ("disorder", C.c_long)]


class LivoxStream:
    """One mml_livox_stream: the aligner's Livox point queue in device memory (Context.livox_stream).  Close it before its context."""

    def __init__(self, ctx, capacity):
        self._ctx = ctx
        self._h = C.c_void_p()
        self._keep = []
        ctx._ck(lib().mml_livox_stream_create(ctx._h, capacity, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            lib().mml_livox_stream_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _held(self, a):
        self._keep.append(a)   # host buffers must outlive the asynchronous copy
        if len(self._keep) > 64:
            self._ctx.synchronize()
            self._keep = self._keep[-1:]

    def push(self, timebase, points):
        """One livox_ros_driver/CustomMsg: its timebase (ns) and its points (LIVOX_DTYPE)."""
        l = np.ascontiguousarray(points)
        assert l.dtype.itemsize == 20
        self._held(l)
        self._ctx._ck(lib().mml_livox_stream_push(self._h, int(timebase), _p(l) if len(l) else None, len(l)))

    def push_wire(self, timebase, wire, n):
        """The same message with its points in wire form: the serialised CustomPoint array, 19 bytes per point."""
        w = np.frombuffer(wire, dtype=np.uint8) if not isinstance(wire, np.ndarray) else np.ascontiguousarray(wire, dtype=np.uint8)
        if len(w) < 19 * n:
            raise ValueError("wire shorter than 19 * n bytes")
        self._held(w)
        self._ctx._ck(lib().mml_livox_stream_push_wire(self._h, int(timebase), _p(w) if n else None, n))

    def state(self):
        """dict(start_stamp, front, tail, disorder); synchronises."""
        st = LivoxStreamState()
        self._ctx._ck(lib().mml_livox_stream_state_get(self._h, C.byref(st)))
        return {"start_stamp": int(st.start_stamp), "front": int(st.front), "tail": int(st.tail), "disorder": int(st.disorder)}

    def reset(self):
        self._ctx._ck(lib().mml_livox_stream_reset(self._h))


class ImuStreamState(C.Structure):
    _fields_ = [("front", C.c_long), ("tail", C.c_long), ("disorder", C.c_long), ("first_stamp", C.c_double), ("last_stamp", C.c_double)]


class ImuStream:
    """One mml_imu_stream: the pose node's IMU message queue in device memory (Context.imu_stream).  Close it before its context."""

    def __init__(self, ctx, capacity):
        self._ctx = ctx
        self._h = C.c_void_p()
        self._keep = []
        ctx._ck(lib().mml_imu_stream_create(ctx._h, capacity, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            lib().mml_imu_stream_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, msgs):
        """Messages as rows of 7 doubles: header stamp (s), angular_velocity xyz, linear_acceleration xyz (message units)."""
        m = _f64(msgs).reshape(-1, 7)
        self._keep.append(m)   # host buffers must outlive the asynchronous copy
        if len(self._keep) > 64:
            self._ctx.synchronize()
            self._keep = self._keep[-1:]
        self._ctx._ck(lib().mml_imu_stream_push(self._h, _p(m) if len(m) else None, len(m)))

    def drop_before(self, t, keep_min=200):
        """fetchImuMsgs' trim: while more than keep_min messages are live and the front one is older than t, drop it."""
        self._ctx._ck(lib().mml_imu_stream_drop_before(self._h, t, keep_min))

    def state(self):
        """dict(front, tail, disorder, first_stamp, last_stamp); synchronises."""
        st = ImuStreamState()
        self._ctx._ck(lib().mml_imu_stream_state_get(self._h, C.byref(st)))
        return {"front": int(st.front), "tail": int(st.tail), "disorder": int(st.disorder), "first_stamp": float(st.first_stamp),
                "last_stamp": float(st.last_stamp)}

    def reset(self):
        self._ctx._ck(lib().mml_imu_stream_reset(self._h))


class Context:
    """One mml_ctx: owns device buffers, maps and a HIP stream for `cfg.max_scans` scan slots."""

    def __init__(self, cfg=None, device=0, **over):
        self.cfg = cfg if cfg is not None else default_config(**over)
        self._h = C.c_void_p()
        rc = lib().mml_create(C.byref(self.cfg), device, C.byref(self._h))
        if rc != MML_OK:
            raise MmlError(rc, "mml_create failed (no HIP device?)" if rc == MML_ERR_NO_DEVICE else "mml_create failed")
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().mml_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != MML_OK:
            raise MmlError(rc, lib().mml_last_error(self._h).decode())

    def synchronize(self):
        self._ck(lib().mml_synchronize(self._h))

    # ---- input / feature extraction (feature_extraction::unionCloudHandler) ----
    def scan_upload(self, slot, velo_xyzi, livox):
        v = _f32(velo_xyzi).reshape(-1, 4) if velo_xyzi is not None else np.zeros((0, 4), np.float32)
        l = np.ascontiguousarray(livox) if livox is not None else np.zeros(0, LIVOX_DTYPE)
        assert l.dtype.itemsize == 20
        self._keep = getattr(self, "_keep", [])
        self._keep.append((v, l))  # host buffers must outlive the async copy
        self._ck(lib().mml_scan_upload(self._h, slot, _p(v), len(v), _p(l), len(l)))
        if len(self._keep) > 4 * self.cfg.max_scans:
            self.synchronize()
            self._keep = self._keep[-self.cfg.max_scans:]

    def scan_upload_batch(self, first, velo_base, n_velo, livox_base, n_livox):
        """count scans in two copies: velo_base (count, max_velo_points, 4) float32, livox_base (count, max_livox_points)
        LIVOX_DTYPE, laid out with the slot stride; n_velo / n_livox: valid points per scan.  The host arrays must stay
        valid until the next synchronising call."""
        nv = np.ascontiguousarray(n_velo, dtype=np.int32)
        nl = np.ascontiguousarray(n_livox, dtype=np.int32)
        count = len(nv)
        v = np.ascontiguousarray(velo_base, dtype=np.float32)
        l = np.ascontiguousarray(livox_base)
        if v.size != count * self.cfg.max_velo_points * 4 or l.size * l.dtype.itemsize != count * self.cfg.max_livox_points * 20:
            raise ValueError("staging arrays must hold count x max points per sensor")
        self._keep = getattr(self, "_keep", [])
        self._keep.append((v, l, nv, nl))
        if len(self._keep) > 4 * self.cfg.max_scans + 8:
            self.synchronize()  # the copies are asynchronous: nothing may be released while one is still in flight
            self._keep = self._keep[-8:]
        self._ck(lib().mml_scan_upload_batch(self._h, first, count, _p(v), _p(nv), _p(l), _p(nl)))

    def scan_upload_pointcloud2(self, slot, data, n_points, point_step, off_x, off_y, off_z, off_intensity, livox):
        """Velodyne part as a sensor_msgs/PointCloud2 payload (bytes / uint8 array), decoded on the device."""
        raw = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        lv = np.ascontiguousarray(livox) if livox is not None else None
        nl = 0 if lv is None else len(lv)
        if len(raw) < n_points * point_step:
            raise ValueError("PointCloud2 payload shorter than n_points * point_step bytes")
        self._ck(lib().mml_scan_upload_pointcloud2(self._h, slot, _p(raw), n_points, point_step, off_x, off_y, off_z, off_intensity,
                                                   _p(lv) if nl else None, nl))
        self.synchronize()

    def scan_upload_wire(self, slot, data, n_points, point_step, off_x, off_y, off_z, off_intensity, livox_wire, n_livox):
        """Both parts in wire form: PointCloud2 payload + the serialised CustomPoint array (19 bytes per point)."""
        raw = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        lw = np.frombuffer(livox_wire, dtype=np.uint8) if not isinstance(livox_wire, np.ndarray) else np.ascontiguousarray(livox_wire, dtype=np.uint8)
        if len(lw) < 19 * n_livox:
            raise ValueError("livox_wire shorter than 19 * n_livox bytes")
        if len(raw) < n_points * point_step:
            raise ValueError("PointCloud2 payload shorter than n_points * point_step bytes")
        self._ck(lib().mml_scan_upload_wire(self._h, slot, _p(raw), n_points, point_step, off_x, off_y, off_z, off_intensity,
                                            _p(lw) if n_livox else None, n_livox))
        self.synchronize()

    def scan_upload_wire_batch(self, first_slot, velo_data, velo_at, n_velo, point_step, offs, livox_data, livox_at, n_livox,
                               livox_record_bytes=19):
        """mml_scan_upload_wire_batch: len(n_velo) union_cloud messages in wire form into slots first_slot .. in ONE call.  Frame i
        is n_velo[i] records of point_step bytes from byte velo_at[i] of velo_data (offs = the byte offsets of x, y, z, intensity,
        the last negative for none) and n_livox[i] records of livox_record_bytes (19: wire form, 20: LIVOX_DTYPE) from byte
        livox_at[i] of livox_data; gaps between the payloads are allowed and travel with them.  A sensor without points may be
        None.  Asynchronous: nothing is synchronised here, the buffers are kept alive by the context."""
        a = wire_batch_pack(velo_data, velo_at, n_velo, point_step, offs, livox_data, livox_at, n_livox, livox_record_bytes)
        self._keep = getattr(self, "_keep", [])
        self._keep.append(a)
        if len(self._keep) > 4 * self.cfg.max_scans + 8:
            self.synchronize()  # the copies are asynchronous: nothing may be released while one is still in flight
            self._keep = self._keep[-8:]
        vd, va, nv, ld, la, nl, lay = a
        self._ck(lib().mml_scan_upload_wire_batch(self._h, first_slot, len(nv), _p(vd), _p(va), _p(nv), *lay[:5], _p(ld), _p(la), _p(nl), lay[5]))

    def time_offset_search(self, velo_xyz, livox_xyz, search_resolution=30, sliced_points=12000, tf=None):
        """estimate_timeoffset's numeric core (unionLidarsAligner.cpp:1077-1153): per-point 1-NN squared distances and
        the sliding-window error; defaults are the reference's (:111-112)."""
        v = np.ascontiguousarray(np.asarray(velo_xyz, np.float32).reshape(-1, 3))
        l = np.ascontiguousarray(np.asarray(livox_xyz, np.float32).reshape(-1, 3))
        t = np.ascontiguousarray(np.asarray(tf, np.float32).reshape(16)) if tf is not None else None
        nn = np.zeros(max(len(l), 1), np.float32)
        cap = max((len(l) - sliced_points) // max(search_resolution, 1) + 2, 1)
        err = np.zeros(cap, np.float64)
        nwin, best, lowest = C.c_int(0), C.c_int(-1), C.c_double(0)
        self._ck(lib().mml_time_offset_search(self._h, _p(v) if len(v) else None, len(v), _p(t) if t is not None else None, _p(l) if len(l) else None,
                                              len(l), search_resolution, sliced_points, _p(nn), _p(err), cap, C.byref(nwin), C.byref(best),
                                              C.byref(lowest)))
        return {"nn_d2": nn[:len(l)], "window_error": err[:nwin.value], "best_window": best.value, "lowest_error": lowest.value}

    def time_offset_search_batch(self, velo_list, livox_list, search_resolution=30, sliced_points=12000, tfs=None):
        """mml_time_offset_search_batch: time_offset_search for a list of (Velodyne, Livox) cloud pairs in one device call; a
        list of the dicts time_offset_search returns.  tfs: None, one 4 x 4 matrix for all problems, or one per problem."""
        velo, vo, livox, lo, tf = time_offset_pack(velo_list, livox_list, tfs)
        n = len(vo) - 1
        rc, bad, nwin = time_offset_plan(vo, lo, search_resolution, sliced_points)
        wo = np.zeros(n + 1, np.int64)     # (C long: 8 bytes on the LP64 hosts ROCm runs on)
        if rc == MML_OK:
            wo[1:] = np.cumsum(nwin)
        nn = np.zeros(max(len(livox), 1), np.float32)
        err = np.zeros(max(int(wo[-1]), 1), np.float64)
        nw = np.zeros(max(n, 1), np.int32)
        best = np.zeros(max(n, 1), np.int32)
        lowest = np.zeros(max(n, 1), np.float64)
        self._ck(lib().mml_time_offset_search_batch(self._h, n, _p(velo) if len(velo) else None, _p(vo), _p(tf), _p(livox) if len(livox) else None,
                                                    _p(lo), search_resolution, sliced_points, _p(nn), _p(err), _p(wo), _p(nw), _p(best), _p(lowest)))
        return [{"nn_d2": nn[lo[i]:lo[i + 1]], "window_error": err[wo[i]:wo[i] + nw[i]], "best_window": int(best[i]),
                 "lowest_error": float(lowest[i])} for i in range(n)]

    def time_offset_estimate_stream(self, stream, livox_begin, livox_end, frames, velo_stamps, tf=None, search_resolution=30,
                                    sliced_points=12000, error_th=1e6):
        """mml_time_offset_estimate_stream: estimate_timeoffset (unionLidarsAligner.cpp:1021-1166) for the Velodyne frames
        `frames` ((n_i, k >= 3) float32 rows x, y, z, ...) against the points [livox_begin, livox_end) of `stream`, FOV selection,
        search and stamps in one call on the resident stream.  velo_stamps: the frames' header stamps (ns); tf: one 4 x 4 matrix or
        None.  Returns a list of dicts: the fields of the frame's TOFS_ROW_DTYPE row (status, n_kept, n_windows, best_window,
        lowest_error, optim_start, time_offset, accepted) plus nn_d2 and window_error (empty for a NO_VELO_IN_FOV row)."""
        data, bo, npts, step = velo_fov_pack(frames)
        n = len(npts)
        vs = np.ascontiguousarray(velo_stamps, dtype=np.uint64)
        if len(vs) != n:
            raise ValueError("%d stamps for %d frames" % (len(vs), n))
        t = np.ascontiguousarray(np.asarray(tf, np.float32).reshape(16)) if tf is not None else None
        L = max(int(livox_end) - int(livox_begin), 0)
        each = (L - sliced_points - 1) // search_resolution + 1 if search_resolution >= 1 and sliced_points >= 1 and L > sliced_points else 0
        wo = (np.arange(n + 1, dtype=np.int64) * each)
        nn = np.zeros(max(n * L, 1), np.float32)
        err = np.zeros(max(int(wo[-1]), 1), np.float64)
        rows = np.zeros(max(n, 1), TOFS_ROW_DTYPE)
        self._ck(lib().mml_time_offset_estimate_stream(self._h, stream._h, int(livox_begin), int(livox_end), n, _p(data) if len(data) else None,
                                                       _p(bo), _p(npts), step, 0, 4, 8, _p(vs), _p(t), search_resolution, sliced_points, error_th,
                                                       _p(nn), _p(err), _p(wo), _p(rows)))
        out = []
        for i in range(n):
            r = {k: rows[k][i].item() for k in TOFS_ROW_DTYPE.names if k != "_pad"}
            ok = r["status"] == TOFS_ROW_OK
            r["nn_d2"] = nn[i * L:(i + 1) * L] if ok else nn[:0]
            r["window_error"] = err[wo[i]:wo[i] + r["n_windows"]]
            out.append(r)
        return out

    def velo_fov_select(self, frames):
        """velo_fov_select(frames, ctx=self): the aligner's FOV selection on the device."""
        return velo_fov_select(frames, ctx=self)

    # ---- the aligner node's frame assembly (unionLidarsAligner.cpp:343-364, :736-868; time-offset mode :513-551, :872-1009) ----
    def imu_stream(self, capacity):
        """An ImuStream of `capacity` messages on this context."""
        return ImuStream(self, capacity)

    def livox_stream(self, capacity):
        """A LivoxStream of `capacity` points on this context."""
        return LivoxStream(self, capacity)

    def union_assemble(self, stream, first_slot, stamps, velo_list, tf=None):
        """mml_union_assemble: frame i = [stamps[i], stamps[i + 1]) (absolute ns) is cut out of `stream` into slot first_slot + i
        together with velo_list[i] (n x 4 float32: x, y, z, intensity) transformed by tf (4 x 4, None: copied).  Returns the
        frames' rows (UNION_FRAME_DTYPE)."""
        st = np.ascontiguousarray(stamps, dtype=np.uint64)
        count = len(st) - 1
        if len(velo_list) != count:
            raise ValueError("%d Velodyne clouds for %d frames" % (len(velo_list), count))
        vs = [_f32(v).reshape(-1, 4) for v in velo_list]
        vo = np.zeros(count + 1, np.int32)
        vo[1:] = np.cumsum([len(v) for v in vs])
        velo = np.ascontiguousarray(np.concatenate(vs + [np.zeros((0, 4), np.float32)]))
        t = np.ascontiguousarray(np.asarray(tf, np.float32).reshape(16)) if tf is not None else None
        rows = np.zeros(max(count, 1), UNION_FRAME_DTYPE)
        self._ck(lib().mml_union_assemble(self._h, stream._h, first_slot, count, _p(st), _p(velo) if len(velo) else None, _p(vo), _p(t), _p(rows)))
        return rows[:count]

    def union_assemble_offset(self, stream, first_slot, starts, sliced_points, velo_list, tf=None):
        """mml_union_assemble_offset, the aligner's time-offset mode (unionLidarsAligner.cpp:513-551, :872-1009): frame i takes up to
        sliced_points points of `stream` from the first one at or after starts[i] (absolute ns: Velodyne stamp - time offset) into
        slot first_slot + i, together with velo_list[i] as in union_assemble.  Returns the frames' rows (UNION_FRAME_DTYPE)."""
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        count = len(st)
        if len(velo_list) != count:
            raise ValueError("%d Velodyne clouds for %d frames" % (len(velo_list), count))
        vs = [_f32(v).reshape(-1, 4) for v in velo_list]
        vo = np.zeros(count + 1, np.int32)
        vo[1:] = np.cumsum([len(v) for v in vs])
        velo = np.ascontiguousarray(np.concatenate(vs + [np.zeros((0, 4), np.float32)]))
        t = np.ascontiguousarray(np.asarray(tf, np.float32).reshape(16)) if tf is not None else None
        rows = np.zeros(max(count, 1), UNION_FRAME_DTYPE)
        self._ck(lib().mml_union_assemble_offset(self._h, stream._h, first_slot, count, _p(st) if count else None, sliced_points,
                                                 _p(velo) if len(velo) else None, _p(vo), _p(t), _p(rows)))
        return rows[:count]

    def scan_raw_download(self, slot):
        """mml_scan_raw_download: the slot's raw input as it stands, (velo n x 4 float32, livox LIVOX_DTYPE)."""
        nv, nl = C.c_int(0), C.c_int(0)
        self._ck(lib().mml_scan_raw_download(self._h, slot, None, 0, None, 0, C.byref(nv), C.byref(nl)))
        v = np.zeros((max(nv.value, 1), 4), np.float32)
        l = np.zeros(max(nl.value, 1), LIVOX_DTYPE)
        self._ck(lib().mml_scan_raw_download(self._h, slot, _p(v), nv.value, _p(l), nl.value, C.byref(nv), C.byref(nl)))
        return v[:nv.value], l[:nl.value]

    def scan_download_pointxyzinormal(self, slot):
        """The fused labelled cloud as 48-byte PointXYZINormal records (the velo_combine / livox_combine payload)."""
        n = C.c_int(0)
        self._ck(lib().mml_scan_download_pointxyzinormal(self._h, slot, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 12), np.float32)
        self._ck(lib().mml_scan_download_pointxyzinormal(self._h, slot, _p(out), n.value, C.byref(n)))
        return out[:n.value]

    def cloud_download_registered(self, first_slot, count, T_wl):
        """The registered clouds of `count` slots (unionPoseEstimation.cpp:896-911): slot first_slot + i moved into the world
        frame by T_wl[i] (transformTobeMapped, 4 x 4; one matrix is enough when count == 1), as a list of (n_i, 12) float32
        arrays of 48-byte PointXYZINormal records -- x y z 1 | 0 0 label 0 | intensity 0 0 0.  The sizing call, then ONE
        data call for all slots (mml_cloud_download_registered_batch)."""
        T = registered_poses(count, T_wl)
        count = len(T)
        n = np.zeros(count, np.int32)
        f = lib().mml_cloud_download_registered_batch
        self._ck(f(self._h, first_slot, count, _p(T), None, 0, _p(n)))
        total = int(n.sum())
        out = np.zeros((max(total, 1), 12), np.float32)
        if total:
            self._ck(f(self._h, first_slot, count, _p(T), _p(out), total, _p(n)))
        ends = np.cumsum(n)
        return [out[e - k:e] for e, k in zip(ends, n)]

    def feature_clouds(self, first_slot, count):
        """The feature node's message for `count` extracted slots (union_cloud.msg:4-9): per slot a tuple of six
        POINTXYZINORMAL_DTYPE arrays in the order of FEATURE_CLOUD_NAMES -- velo_corner, velo_surface, velo_combine, livox_corner,
        livox_surface, livox_combine.  The sizing call, then ONE data call for all slots (mml_feature_clouds_download_batch)."""
        count = int(count)
        if count < 1:
            raise ValueError("count must be at least 1, not %d" % count)
        n = np.zeros(6 * count, np.int32)
        f = lib().mml_feature_clouds_download_batch
        self._ck(f(self._h, first_slot, count, None, 0, _p(n)))
        total = int(n.sum())
        out = np.zeros(max(total, 1), POINTXYZINORMAL_DTYPE)
        if total:
            self._ck(f(self._h, first_slot, count, _p(out), total, _p(n)))
        ends = np.cumsum(n)
        clouds = [out[e - k:e] for e, k in zip(ends, n)]
        return [tuple(clouds[6 * i:6 * i + 6]) for i in range(count)]

    def cloud_upload(self, slot, records, n_velo=None):
        """A labelled fused cloud (n x 12 float32 = 48-byte PointXYZINormal records, velo_combine then livox_combine)
        into a slot: the PoseEstimation side of /union_feature_cloud."""
        rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 12)
        nv = len(rec) if n_velo is None else int(n_velo)
        self._ck(lib().mml_cloud_upload(self._h, slot, _p(rec) if len(rec) else None, len(rec), nv))

    def pose_ingest(self, first_slot, clouds, n_points=None, rows=None, **opts):
        """mml_pose_ingest_batch: n union_cloud messages into slots first_slot .. in ONE call, with the pose node's decision per
        message (merge the Livox cloud or not, fast rotation, the frame dropped for want of IMU messages).  `clouds`: the list of
        six-array tuples Context.feature_clouds returns, or the raw block (records as POINTXYZINORMAL_DTYPE, (n, 12) float32 or
        bytes) with n_points (n, 6).  rows: the IMU_INTERVAL_DTYPE rows of imu_fetch_batch, or None (IMU_Mode 0).  opts:
        hori_rotate_th, velo_rotate_th, velo_only_mode, first_frame.  Returns the rows (POSE_INGEST_ROW_DTYPE)."""
        block, n, r, o = pose_ingest_pack(clouds, n_points, rows, opts)
        out = np.zeros(max(len(n), 1), POSE_INGEST_ROW_DTYPE)
        self._ck(lib().mml_pose_ingest_batch(self._h, first_slot, len(n), _p(block) if block.size else None, _p(n), _p(r), C.byref(o), _p(out)))
        return out[:len(n)]

    def gicp_align(self, src, tgt, T0=None):
        """icp_ext_matching on plain clouds: returns (converged, T 4x4 float32, GicpInfo)."""
        src = _f32(src).reshape(-1, 3)
        tgt = _f32(tgt).reshape(-1, 3)
        T = np.ascontiguousarray(np.eye(4, dtype=np.float32) if T0 is None else np.asarray(T0, np.float32).reshape(4, 4).copy())
        conv, info = C.c_int(0), GicpInfo()
        self._ck(lib().mml_gicp_align(self._h, _p(src) if len(src) else None, len(src), _p(tgt) if len(tgt) else None, len(tgt), _p(T), C.byref(conv),
                                      C.byref(info)))
        return bool(conv.value), T, info

    def gicp_align_opts(self, src, tgt, max_iterations=10, transformation_epsilon=1e-6, max_correspondence_distance=0.0, T0=None):
        """mml_gicp_align_opts: gicp_align with PCL's three settings as arguments (the defaults are gicp_align's); returns
        (converged, T 4x4 float32, GicpInfo)."""
        src = _f32(src).reshape(-1, 3)
        tgt = _f32(tgt).reshape(-1, 3)
        T = np.ascontiguousarray(np.eye(4, dtype=np.float32) if T0 is None else np.asarray(T0, np.float32).reshape(4, 4).copy())
        opts = GicpOpts(int(max_iterations), float(transformation_epsilon), float(max_correspondence_distance))
        conv, info = C.c_int(0), GicpInfo()
        self._ck(lib().mml_gicp_align_opts(self._h, _p(src) if len(src) else None, len(src), _p(tgt) if len(tgt) else None, len(tgt), C.byref(opts),
                                           _p(T), C.byref(conv), C.byref(info)))
        return bool(conv.value), T, info

    def debug_gicp(self, op, src=None, tgt=None, cov_src=None, cov_tgt=None, T=None, corr=None, maha=None, x=None, gate2=0.0, grad=True,
                   max_iterations=10, transformation_epsilon=1e-6):
        """mml_debug_gicp (a test hook): one piece of the device's GICP on the caller's inputs; include/mmloam_hip.h lists the
        operations.  Returns, by op: COV (cov n x 3 x 3, ids n x 20); CORR (corr n, maha n x 3 x 3); EVAL (f K x 2, g K x 2 x 6: lane 0's
        copy and the last lane's); INTERP alpha[n]; QUAD (count n, roots n x 2); STATE (T n x 4 x 4 float32, x n x 6);
        ROUND a dict of T, converged, failed, nr, evals, fobj, delta."""
        io = GicpDebug()
        keep = []

        def arr(a, dt, width):
            if a is None:
                return None, 0
            a = np.ascontiguousarray(a, dtype=dt).reshape(-1, width)
            keep.append(a)
            return _p(a) if a.size else None, len(a)
        io.src, io.n_src = arr(src, np.float32, 3)
        io.tgt, io.n_tgt = arr(tgt, np.float32, 3)
        io.cov_src, io.cov_tgt = arr(cov_src, np.float64, 9)[0], arr(cov_tgt, np.float64, 9)[0]
        io.T = arr(T, np.float32, 16)[0]
        io.corr, io.maha = arr(corr, np.int32, 1)[0], arr(maha, np.float64, 9)[0]
        io.x, io.k = arr(x, np.float64, {GICP_DBG_INTERP: 8, GICP_DBG_QUAD: 3}.get(op, 6))
        io.gate2, io.grad = float(gate2), int(bool(grad))
        io.max_iterations, io.transformation_epsilon = int(max_iterations), float(transformation_epsilon)
        ns, nt, k = max(io.n_src, 1), max(io.n_tgt, 1), max(io.k, 1)
        nd = {GICP_DBG_COV: 9 * nt, GICP_DBG_CORR: 9 * ns, GICP_DBG_EVAL: 14 * k, GICP_DBG_INTERP: k, GICP_DBG_QUAD: 3 * k,
              GICP_DBG_STATE: 6 * k, GICP_DBG_ROUND: 2}.get(op, 1)
        ni = {GICP_DBG_COV: 20 * nt, GICP_DBG_CORR: ns, GICP_DBG_ROUND: 4}.get(op, 1)
        od, oi, of = np.zeros(nd), np.zeros(ni, np.int32), np.zeros(16 * k, np.float32)
        io.out_d, io.out_i, io.out_f = _p(od), _p(oi), _p(of)
        self._ck(lib().mml_debug_gicp(self._h, op, C.byref(io)))
        if op == GICP_DBG_COV:
            return od.reshape(-1, 3, 3), oi.reshape(-1, 20)
        if op == GICP_DBG_CORR:
            return oi, od.reshape(-1, 3, 3)
        if op == GICP_DBG_EVAL:
            o = od.reshape(-1, 2, 7)
            return o[:, :, 0], o[:, :, 1:]
        if op == GICP_DBG_INTERP:
            return od
        if op == GICP_DBG_QUAD:
            o = od.reshape(-1, 3)
            return o[:, 0].astype(int), o[:, 1:]
        if op == GICP_DBG_STATE:
            return of.reshape(-1, 4, 4), od.reshape(-1, 6)
        return dict(T=of[:16].reshape(4, 4), converged=int(oi[0]), failed=int(oi[1]), nr=int(oi[2]), evals=int(oi[3]), fobj=od[0], delta=od[1])

    def cloud_crop_voxel(self, xyzi, far_th, leaf, out=None):
        """mml_cloud_crop_voxel: removeFarPointCloud(far_th) + pcl::VoxelGrid(leaf) of an n x 4 (x, y, z, intensity) cloud on the
        device; returns (m x 4 float32, unfiltered).  out=None: a sizing call first, then room for exactly the result; else the
        records go into `out` (k x 4 float32, C order; MmlError MML_ERR_CAPACITY, nothing written, when k is too small)."""
        xyzi = _f32(xyzi).reshape(-1, 4)
        f = lib().mml_cloud_crop_voxel
        n, unf = C.c_int(0), C.c_int(0)
        a = (self._h, _p(xyzi) if len(xyzi) else None, len(xyzi), far_th, leaf)
        if out is None:
            self._ck(f(*a, None, 0, C.byref(n), C.byref(unf)))
            out = np.zeros((max(n.value, 1), 4), np.float32)
            cap = n.value
        else:
            assert out.dtype == np.float32 and out.flags.c_contiguous and out.ndim == 2 and out.shape[1] == 4
            cap = len(out)
        self._ck(f(*a, _p(out), cap, C.byref(n), C.byref(unf)))
        return out[:n.value], bool(unf.value)

    def aligner_calibrate(self, hori_xyzi, velo_xyzi, hori_tf=None, velo_hori_tf=None):
        """mml_aligner_calibrate: calibratePCLICP and its call site (unionLidarsAligner.cpp:221-270) on the integrated Livox cloud
        and the newest Velodyne cloud, both n x 4; returns (converged, hori_tf, velo_hori_tf, CalibInfo).  The two matrices
        (identity unless given) come back untouched when the alignment does not converge."""
        h = _f32(hori_xyzi).reshape(-1, 4)
        v = _f32(velo_xyzi).reshape(-1, 4)
        mats = [np.ascontiguousarray(np.eye(4, dtype=np.float32) if m is None else np.asarray(m, np.float32).reshape(4, 4).copy())
                for m in (hori_tf, velo_hori_tf)]
        conv, info = C.c_int(0), CalibInfo()
        self._ck(lib().mml_aligner_calibrate(self._h, _p(h) if len(h) else None, len(h), _p(v) if len(v) else None, len(v), _p(mats[0]), _p(mats[1]),
                                             C.byref(conv), C.byref(info)))
        return bool(conv.value), mats[0], mats[1], info

    def gicp_refresh(self, slot, extrinsic, apply=True):
        """unionCloudHandler's extrinsic refresh (:302-318) on a slot extracted without an extrinsic."""
        T = np.ascontiguousarray(np.asarray(extrinsic, np.float32).reshape(4, 4).copy())
        ref, info = C.c_int(0), GicpInfo()
        self._ck(lib().mml_gicp_refresh(self._h, slot, _p(T), 1 if apply else 0, C.byref(ref), C.byref(info)))
        return bool(ref.value), T, info

    def gicp_align_batch(self, pairs, T0=None):
        """mml_gicp_align_batch: gicp_align for a list of (src, tgt) pairs in one device call; a list of (converged, T, GicpInfo)."""
        src, so, tgt, to, T = gicp_pack_pairs(pairs, T0)
        n = len(pairs)
        conv = np.zeros(max(n, 1), np.int32)
        info = (GicpInfo * max(n, 1))()
        self._ck(lib().mml_gicp_align_batch(self._h, n, _p(src) if len(src) else None, _p(so), _p(tgt) if len(tgt) else None, _p(to), _p(T), _p(conv),
                                            C.cast(info, C.c_void_p)))
        return [(bool(conv[i]), T[i], info[i]) for i in range(n)]

    def gicp_refresh_batch(self, first_slot, count, extrinsic, chain=True, apply=True):
        """mml_gicp_refresh_batch: the refresh of `count` extracted slots in one device call.  chain=True: `extrinsic` is the one
        persistent 4 x 4 extri_mtx carried through the frames; chain=False: count matrices, one per slot.  Returns
        (refreshed[count] bool, T[count, 4, 4] float32 -- the matrix held after (and applied to) each frame --, [GicpInfo])."""
        n = max(int(count), 1)
        T = np.zeros((n, 4, 4), np.float32)
        e = np.asarray(extrinsic, np.float32)
        if chain:
            T[0] = e.reshape(-1)[:16].reshape(4, 4)
        else:
            T[:] = e.reshape(n, 4, 4)
        ref = np.zeros(n, np.int32)
        info = (GicpInfo * n)()
        self._ck(lib().mml_gicp_refresh_batch(self._h, first_slot, count, _p(T), 1 if chain else 0, 1 if apply else 0, _p(ref),
                                              C.cast(info, C.c_void_p)))
        return ref[:count].astype(bool), T[:count], list(info)[:count]

    def extract(self, first=0, count=1, livox_extrinsic=None):
        e = _f32(livox_extrinsic).reshape(16) if livox_extrinsic is not None else None
        self._ck(lib().mml_extract(self._h, first, count, _p(e)))

    def scan_info(self, slot):
        info = ScanInfo()
        self._ck(lib().mml_scan_info_get(self._h, slot, C.byref(info)))
        return info

    def scan_download(self, slot):
        info = self.scan_info(slot)
        n = info.n_points
        xyzi = np.zeros((max(n, 1), 4), np.float32)
        rel = np.zeros(max(n, 1), np.float32)
        line = np.zeros(max(n, 1), np.uint8)
        label = np.zeros(max(n, 1), np.uint8)
        self._ck(lib().mml_scan_download(self._h, slot, _p(xyzi), _p(rel), _p(line), _p(label), max(n, 1)))
        return dict(xyzi=xyzi[:n], reltime=rel[:n], ring=line[:n].astype(np.int32), label=label[:n].astype(np.int32),
                    info=info)

    def detect_line(self, pts):
        """Twin of feature_extraction::detectFeaturePoints: returns (sharp idx, flat idx, CloudFeatureFlag)."""
        pts = _f32(pts).reshape(-1, 4)
        n = len(pts)
        sharp = np.zeros(max(n, 1), np.int32)
        flat = np.zeros(max(n, 1), np.int32)
        flags = np.zeros(max(n, 1), np.int32)
        ns, nf = C.c_int(0), C.c_int(0)
        self._ck(lib().mml_detect_line(self._h, _p(pts), n, _p(sharp), C.byref(ns), _p(flat), C.byref(nf), _p(flags)))
        return sharp[:ns.value].copy(), flat[:nf.value].copy(), flags[:n].copy()

    # ---- RemoveLidarDistortion ----
    def undistort(self, first, count, dR, dt):
        dR = _f64(dR).reshape(count, 9)
        dt = _f64(dt).reshape(count, 3)
        self._ck(lib().mml_undistort(self._h, first, count, _p(dR), _p(dt)))

    # ---- Estimator::EstimateLidarPose pieces ----
    def downsample(self, first=0, count=1):
        self._ck(lib().mml_downsample(self._h, first, count))

    def features_download(self, slot, kind):
        n = C.c_int(0)
        self._ck(lib().mml_features_download(self._h, slot, kind, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 3), np.float32)
        self._ck(lib().mml_features_download(self._h, slot, kind, _p(out), max(n.value, 1), C.byref(n)))
        return out[:n.value]

    def features_count(self, slot, kind):
        """Points in the slot's down-sampled stack of `kind`, without the copy."""
        n = C.c_int(0)
        self._ck(lib().mml_features_download(self._h, slot, kind, None, 0, C.byref(n)))
        return n.value

    def features_upload(self, slot, kind, xyz):
        xyz = _f32(xyz).reshape(-1, 3)
        self._ck(lib().mml_features_upload(self._h, slot, kind, _p(xyz), len(xyz)))

    def map_set_local(self, kind, xyz):
        xyz = _f32(xyz).reshape(-1, 3)
        self._ck(lib().mml_map_set_local(self._h, kind, _p(xyz), len(xyz)))

    def map_increment_local(self, slot, T_wl):
        """Estimator::MapIncrementLocal on the device; returns the new (corner, surf) local map sizes."""
        nc, ns = C.c_int(0), C.c_int(0)
        T = _f64(T_wl).reshape(16)
        self._ck(lib().mml_map_increment_local(self._h, slot, _p(T), C.byref(nc), C.byref(ns)))
        return nc.value, ns.value

    def map_local_reset(self):
        self._ck(lib().mml_map_local_reset(self._h))

    def _download(self, f, head, shapes, tail=(), count=C.c_int):
        """The two-call download f(handle, *head, *buffers, capacity, &n, *tail): with null buffers it reports n, then it fills
        one buffer of n rows per entry of shapes -- (columns, or None for a flat array; dtype).  Returns the buffers, n rows each."""
        n = count(0)
        self._ck(f(self._h, *head, *[None] * len(shapes), 0, C.byref(n), *tail))
        rows = max(n.value, 1)
        out = [np.zeros(rows if w is None else (rows, w), t) for w, t in shapes]
        if n.value:
            self._ck(f(self._h, *head, *[_p(a) for a in out], n.value, C.byref(n), *tail))
        return [a[:n.value] for a in out]

    def map_local_download(self, kind):
        return self._download(lib().mml_map_local_download, (int(kind),), [(3, np.float32)])[0]

    # ---- the world map: the registered clouds voxel-merged on the device, n maps (include/mmloam_hip.h, "The world map") ----
    def world_map_create(self, n_maps, leaf, capacity_voxels, surfels=False):
        """n_maps (1 .. 1024) voxel maps of leaf size `leaf` in one table of capacity_voxels voxels; once per context.
        surfels=True: a surfel map (MML_WM_SURFELS), 76 bytes per table position instead of 28; world_map_moments and
        world_map_surfels read it."""
        self._wm_leaf, self._wm_surfels = float(leaf), bool(surfels)   # (opts=None of world_map_associate / _localize; world_map_export)
        if surfels:
            self._ck(lib().mml_world_map_create_opts(self._h, int(n_maps), float(leaf), int(capacity_voxels), MML_WM_SURFELS))
        else:
            self._ck(lib().mml_world_map_create(self._h, int(n_maps), float(leaf), int(capacity_voxels)))

    def _world_map_rows(self, f, map, width):
        return self._download(f, (int(map),), [(width, np.float32)], count=C.c_long)[0]

    def world_map_moments(self, map):
        """The raw accumulators of a surfel map's voxels in the order of world_map_download: (n, 12) float32
        sdx sdy sdz vx | sxx sxy sxz vy | syy syz szz vz (offsets from the voxel's centre, their products, the view sum)."""
        return self._world_map_rows(lib().mml_world_map_download_moments, map, 12)

    def world_map_surfels(self, map):
        """The surfels of a surfel map's voxels in the order of world_map_download: (n, 8) float32 nx ny nz | l0 l1 l2 |
        planarity linearity; eight zeros for a voxel of fewer than 3 points."""
        return self._world_map_rows(lib().mml_world_map_download_surfels, map, 8)

    def world_map_destroy(self):
        self._ck(lib().mml_world_map_destroy(self._h))

    def world_map_reset(self, map=-1):
        """Empties one map, or all (-1)."""
        self._ck(lib().mml_world_map_reset(self._h, int(map)))

    def world_map_add(self, first_slot, maps, T_wl, label_mask=7):
        """Slot first_slot + i into map maps[i] (-1: skipped) at T_wl[i] (4 x 4), the points whose label's bit is set in
        label_mask: ONE mml_world_map_add call.  Returns its WorldMapInfo."""
        m = np.ascontiguousarray(maps, dtype=np.int32).reshape(-1)
        T = registered_poses(len(m), T_wl)
        info = WorldMapInfo()
        self._ck(lib().mml_world_map_add(self._h, int(first_slot), len(m), _p(m), _p(T), int(label_mask), C.byref(info)))
        return info

    def world_map_size(self, map=-1):
        """The voxels of one map, or of all (-1)."""
        n = C.c_long(0)
        self._ck(lib().mml_world_map_size(self._h, int(map), C.byref(n)))
        return n.value

    def world_map_download(self, map, counts=False):
        """The voxels of one map in ascending key order: (n, 4) float32 centroids x, y, z, intensity; counts=True: and the
        (n,) int32 point counts.  The sizing call, then one data call."""
        out, cnt = self._download(lib().mml_world_map_download, (int(map),), [(4, np.float32), (None, np.int32)], count=C.c_long)
        return (out, cnt) if counts else out

    def world_map_export(self, map):
        """One map as it is stored, in the order of world_map_download: dict(ijk (n, 3) int32 voxel indices, sums (n, 4) float32
        (the sums, not the centroids), counts (n,) int32, moments (n, 12) float32 or None on a plain map)."""
        L = lib()
        n = C.c_long(0)
        self._ck(L.mml_world_map_export(self._h, int(map), None, None, None, None, 0, C.byref(n)))
        rows = n.value
        ijk, sums, counts = np.zeros((rows, 3), np.int32), np.zeros((rows, 4), np.float32), np.zeros(rows, np.int32)
        mom = np.zeros((rows, 12), np.float32) if getattr(self, "_wm_surfels", False) else None   # (a plain map takes no moments)
        if rows:
            self._ck(L.mml_world_map_export(self._h, int(map), _p(ijk), _p(sums), _p(counts), _p(mom), rows, C.byref(n)))
        return dict(ijk=ijk, sums=sums, counts=counts, moments=mom)

    def world_map_import(self, map, ijk, sums, counts, moments=None):
        """The inverse of world_map_export (its dict unpacked): n voxels that the map does not hold yet."""
        ijk = np.ascontiguousarray(ijk, np.int32).reshape(-1, 3)
        sums = _f32(sums).reshape(-1, 4)
        counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
        mom = None if moments is None else _f32(moments).reshape(-1, 12)
        if len(sums) != len(ijk) or len(counts) != len(ijk) or (mom is not None and len(mom) != len(ijk)):
            raise ValueError("ijk, sums, counts and moments must have one row per voxel")
        self._ck(lib().mml_world_map_import(self._h, int(map), len(ijk), _p(ijk), _p(sums), _p(counts), _p(mom)))

    def world_map_associate(self, first, maps, T_wl, opts=None, stats=True):
        """Plane factors for the surf stacks of slots first + i from the surfels of map maps[i] (-1: skipped): ONE launch.
        opts: a WmAssocOpts (wm_assoc_opts(leaf, ...); None: the defaults for the map's leaf).  stats=False: no statistics are read
        back (the poses and map numbers are staged before the call returns)."""
        m = np.ascontiguousarray(maps, dtype=np.int32).reshape(-1)
        T = _f64(T_wl).reshape(len(m), 16)
        st = (AssocStats * len(m))() if stats else None
        if opts is None:
            opts = wm_assoc_opts(getattr(self, "_wm_leaf", 1.0))
        self._ck(lib().mml_world_map_associate(self._h, int(first), len(m), _p(m), _p(T), C.byref(opts), st))
        return list(st) if stats else None

    def world_map_localize(self, first, maps, exTlb, P, Q, opts=None):
        """mml_world_map_localize: Context.estimate's loop against the surfel map.  opts: a WmLocalizeOpts
        (wm_localize_opts(leaf, ...)).  Returns P, Q, [EstimateInfo]."""
        m = np.ascontiguousarray(maps, dtype=np.int32).reshape(-1)
        P = _f64(P).reshape(len(m), 3).copy()
        Q = _f64(Q).reshape(len(m), 4).copy()
        info = (EstimateInfo * len(m))()
        if opts is None:
            opts = wm_localize_opts(getattr(self, "_wm_leaf", 1.0))
        self._ck(lib().mml_world_map_localize(self._h, int(first), len(m), _p(m), _p(_f64(exTlb).reshape(16)), _p(P), _p(Q),
                                              C.byref(opts), info))
        return P, Q, list(info)

    def world_map_score(self, first, maps, T_wl, opts=None):
        """mml_world_map_score: the surf stacks of slots first + i against map maps[i] (-1: zeros) at every hypothesis of T_wl
        (len(maps), H, 4, 4), ONE launch.  opts: a WmScoreOpts (wm_score_opts(leaf, ...)).  Returns a (len(maps), H) structured
        array (score_q, n_match, n_scored)."""
        m = np.ascontiguousarray(maps, dtype=np.int32).reshape(-1)
        T = _f64(T_wl).reshape(len(m), -1, 16)
        out = np.zeros((len(m), T.shape[1]), WM_SCORE_DT)
        if opts is None:
            opts = wm_score_opts(getattr(self, "_wm_leaf", 1.0))
        self._ck(lib().mml_world_map_score(self._h, int(first), len(m), _p(m), T.shape[1], _p(T), C.byref(opts), _p(out)))
        return out

    def world_map_relocalize(self, first, maps, exTlb, P, Q, opts=None):
        """mml_world_map_relocalize: the coarse-to-fine search around the seed poses P, Q, ending in world_map_localize.  opts: a
        WmRelocOpts (wm_reloc_opts(leaf, ...)).  Returns P, Q, [WmRelocInfo]."""
        m = np.ascontiguousarray(maps, dtype=np.int32).reshape(-1)
        P = _f64(P).reshape(len(m), 3).copy()
        Q = _f64(Q).reshape(len(m), 4).copy()
        info = (WmRelocInfo * len(m))()
        if opts is None:
            opts = wm_reloc_opts(getattr(self, "_wm_leaf", 1.0))
        self._ck(lib().mml_world_map_relocalize(self._h, int(first), len(m), _p(m), _p(_f64(exTlb).reshape(16)), _p(P), _p(Q),
                                                C.byref(opts), info))
        return P, Q, list(info)

    def world_map_index_box(self, lo_xyz, hi_xyz):
        """wm_index_box for this context's world map: the index box (lo, hi) of the metric box [lo_xyz, hi_xyz]."""
        return wm_index_box(self._wm_leaf, lo_xyz, hi_xyz)

    def world_map_evict(self, rules, rows=True, dry=False):
        """mml_world_map_evict: rules, a list of WmEvictRule (wm_evict_rule(map, mode, lo, hi, min_count)), at most one per map, in
        ONE call.  Returns the list of WmEvictInfo, one per rule; with rows=True (and not dry) also {map: dict(ijk, sums, counts,
        moments)} of the evicted voxels per named map, each as world_map_import takes it (world_map_import(map, **rows[map])); the
        arrays are sized by a dry run first.  rows=False drops the evicted voxels.  dry=True: counts only, nothing is written."""
        L = lib()
        arr = (WmEvictRule * len(rules))(*rules)
        info = (WmEvictInfo * len(rules))()
        n = C.c_long(0)
        if dry or not rows:
            self._ck(L.mml_world_map_evict(self._h, len(rules), arr, MML_WM_EVICT_DRY if dry else 0, info, 0, None, None, None, None, None,
                                           C.byref(n)))
            return list(info)
        self._ck(L.mml_world_map_evict(self._h, len(rules), arr, MML_WM_EVICT_DRY, info, 0, None, None, None, None, None, C.byref(n)))
        cap = max(n.value, 1)
        omap, ijk, sums, counts = np.zeros(cap, np.int32), np.zeros((cap, 3), np.int32), np.zeros((cap, 4), np.float32), np.zeros(cap, np.int32)
        mom = np.zeros((cap, 12), np.float32) if getattr(self, "_wm_surfels", False) else None
        self._ck(L.mml_world_map_evict(self._h, len(rules), arr, 0, info, cap, _p(omap), _p(ijk), _p(sums), _p(counts), _p(mom), C.byref(n)))
        out = {}
        for r, i in zip(rules, info):
            a, b = i.first_row, i.first_row + i.n_evicted
            out[int(r.map)] = dict(ijk=ijk[a:b].copy(), sums=sums[a:b].copy(), counts=counts[a:b].copy(),
                                   moments=None if mom is None else mom[a:b].copy())
        return list(info), out

    # ---- map banks: further local maps, every slot matched against its own (include/mmloam_hip.h, "map banks") ----
    def map_banks(self, n):
        """Creates n banks (n = 0: releases them and unbinds every slot)."""
        if n == 0:
            self._ck(lib().mml_map_banks_destroy(self._h))
        else:
            self._ck(lib().mml_map_banks_create(self._h, n))

    def bind_banks(self, first, banks):
        """banks[i]: the bank of slot first + i, -1 the context's own map; stays until it is changed."""
        b = np.ascontiguousarray(banks, dtype=np.int32).reshape(-1)
        self._ck(lib().mml_slot_bind_bank(self._h, first, len(b), _p(b)))

    def slot_banks(self, first, count):
        b = np.zeros(count, np.int32)
        self._ck(lib().mml_slot_bank_get(self._h, first, count, _p(b)))
        return b

    def bank_set_local(self, bank, kind, xyz):
        xyz = _f32(xyz).reshape(-1, 3)
        self._ck(lib().mml_map_bank_set_local(self._h, bank, kind, _p(xyz), len(xyz)))

    def bank_reset(self, bank):
        self._ck(lib().mml_map_bank_reset(self._h, bank))

    def bank_download(self, bank, kind):
        return self._download(lib().mml_map_bank_download, (int(bank), int(kind)), [(3, np.float32)])[0]

    def bank_increment(self, banks, slots, T_wl, segmented=False):
        """Estimator::MapIncrementLocal for len(banks) distinct banks in one call: bank banks[i] grows by the stacks of slot
        slots[i] at T_wl[i] (4 x 4).  Returns the new (corner, surf) map sizes, one pair of arrays entry per bank.
        segmented=True: mml_map_bank_increment_segmented -- the same banks, bit for bit, from one chain of launches with 2 + R
        host synchronisations whatever len(banks) is; a slot without a stack is refused before any bank changes."""
        b = np.ascontiguousarray(banks, dtype=np.int32).reshape(-1)
        s = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        T = _f64(T_wl).reshape(-1, 16)
        if not (len(b) == len(s) == len(T)):
            raise ValueError("one slot and one pose per bank")
        nc, ns = np.zeros(max(len(b), 1), np.int32), np.zeros(max(len(b), 1), np.int32)
        call = lib().mml_map_bank_increment_segmented if segmented else lib().mml_map_bank_increment
        self._ck(call(self._h, len(b), _p(b), _p(s), _p(T), _p(nc), _p(ns)))
        return nc[:len(b)], ns[:len(b)]

    def debug_bank_increment_budget(self, points):
        """mml_debug_bank_increment_budget (a test hook): the ring points a segmented bank_increment works on at a time."""
        self._ck(lib().mml_debug_bank_increment_budget(self._h, int(points)))

    # ---- a bank's global cube map: its own MAP_MANAGER store and match copy (include/mmloam_hip.h, "map banks") ----
    def bank_set_global(self, bank, kind, xyz, cube, cen=None):
        """map_set_global on bank `bank`; an empty cloud removes that bank's cube map."""
        xyz = _f32(xyz).reshape(-1, 3)
        cube = np.ascontiguousarray(cube, dtype=np.int32).reshape(-1)
        if len(cube) != len(xyz):
            raise ValueError("one cube index per point")
        cen_p = None if cen is None else _p(np.ascontiguousarray(cen, dtype=np.int32))
        self._ck(lib().mml_map_bank_set_global(self._h, bank, kind, _p(xyz), _p(cube), len(xyz), cen_p))

    def bank_global_append(self, banks, slots, T_wl, segmented=False):
        """map_global_append for len(banks) distinct banks in one call: the stacks of slot slots[i] at T_wl[i] (4 x 4) go to
        the pending clouds of bank banks[i].  segmented=True: mml_map_bank_global_append_segmented -- one read-back of all
        stack sizes, one launch for all banks."""
        b = np.ascontiguousarray(banks, dtype=np.int32).reshape(-1)
        s = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        T = _f64(T_wl).reshape(-1, 16)
        if not (len(b) == len(s) == len(T)):
            raise ValueError("one slot and one pose per bank")
        call = lib().mml_map_bank_global_append_segmented if segmented else lib().mml_map_bank_global_append
        self._ck(call(self._h, len(b), _p(b), _p(s), _p(T)))

    def bank_global_increment(self, banks, T_wl, segmented=False):
        """map_global_increment for len(banks) distinct banks in one call, bank banks[i] at T_wl[i].  Returns the live (corner,
        surf) store sizes, one pair of arrays entry per bank.  segmented=True: mml_map_bank_global_increment_segmented -- the
        same banks, bit for bit, from one chain of launches with 3 + R host synchronisations whatever len(banks) is; every
        refusal leaves every bank of the call as it was."""
        b = np.ascontiguousarray(banks, dtype=np.int32).reshape(-1)
        T = _f64(T_wl).reshape(-1, 16)
        if len(b) != len(T):
            raise ValueError("one pose per bank")
        nc, ns = np.zeros(max(len(b), 1), np.int32), np.zeros(max(len(b), 1), np.int32)
        call = lib().mml_map_bank_global_increment_segmented if segmented else lib().mml_map_bank_global_increment
        self._ck(call(self._h, len(b), _p(b), _p(T), _p(nc), _p(ns)))
        return nc[:len(b)], ns[:len(b)]

    def bank_global_increment_budget(self, points):
        """mml_debug_bank_global_increment_budget (a test hook): the points a segmented bank_global_increment works on at a time."""
        self._ck(lib().mml_debug_bank_global_increment_budget(self._h, int(points)))

    def bank_global_download(self, bank, kind):
        return self._cube_download(lib().mml_map_bank_global_download, (int(bank), int(kind)))

    def bank_global_reset(self, bank):
        self._ck(lib().mml_map_bank_global_reset(self._h, bank))

    def map_global_append(self, slot, T_wl):
        self._ck(lib().mml_map_global_append(self._h, slot, _p(_f64(T_wl).reshape(16))))

    def map_global_increment(self, T_wl):
        """MAP_MANAGER::MapIncrement on the device; returns the live (corner, surf) store sizes."""
        nc, ns = C.c_int(0), C.c_int(0)
        self._ck(lib().mml_map_global_increment(self._h, _p(_f64(T_wl).reshape(16)), C.byref(nc), C.byref(ns)))
        return nc.value, ns.value

    def _cube_download(self, f, head):
        cen = np.zeros(3, np.int32)
        xyz, cube = self._download(f, head, [(3, np.float32), (None, np.int32)], tail=(_p(cen),))
        return xyz, cube, cen

    def map_global_download(self, kind):
        return self._cube_download(lib().mml_map_global_download, (int(kind),))

    def map_global_reset(self):
        self._ck(lib().mml_map_global_reset(self._h))

    def map_set_global(self, kind, xyz, cube, cen=None):
        """Cube store of the global map (a12): xyz (m, 3) and the ToIndex cube of every point."""
        xyz = _f32(xyz).reshape(-1, 3)
        cube = np.ascontiguousarray(cube, dtype=np.int32).reshape(-1)
        if len(cube) != len(xyz):
            raise ValueError("one cube index per point")
        cen_p = None if cen is None else _p(np.ascontiguousarray(cen, dtype=np.int32))
        self._ck(lib().mml_map_set_global(self._h, kind, _p(xyz), _p(cube), len(xyz), cen_p))

    def knn5(self, kind, q, max_d2=np.inf):
        q = _f32(q).reshape(-1, 3)
        idx = np.zeros((len(q), 5), np.int32)
        d2 = np.zeros((len(q), 5), np.float32)
        md = np.float32(min(max_d2, 3.0e38))
        self._ck(lib().mml_knn5(self._h, kind, _p(q), len(q), md, _p(idx), _p(d2)))
        return idx, d2

    def associate(self, first, count, T_wl, thres_dist, stats=True):
        """stats=False: enqueue only (no read-back, no synchronisation) -- what a caller does that goes straight on to
        mml_solve on the same slots."""
        T = _f64(T_wl).reshape(count, 16)
        if not stats:
            self._keep_T = T                              # the poses are staged before the call returns; kept anyway
            self._ck(lib().mml_associate(self._h, first, count, _p(T), thres_dist, None))
            return None
        st = (AssocStats * count)()
        self._ck(lib().mml_associate(self._h, first, count, _p(T), thres_dist, st))
        return list(st)

    def factors_download(self, slot, kind):
        n = C.c_int(0)
        self._ck(lib().mml_factors_download(self._h, slot, kind, None, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 10))
        src = np.zeros(max(n.value, 1), np.int32)
        self._ck(lib().mml_factors_download(self._h, slot, kind, _p(out), _p(src), max(n.value, 1), C.byref(n)))
        return out[:n.value], src[:n.value]

    def factors_upload(self, slot, kind, rec):
        rec = _f64(rec).reshape(-1, 10)
        self._ck(lib().mml_factors_upload(self._h, slot, kind, _p(rec), len(rec)))

    def linearize(self, slot, x, T_bl, w_tan=0.0, huber=0.1 / 1.5e-3):
        H = np.zeros((6, 6))
        g = np.zeros(6)
        c = C.c_double(0)
        self._ck(lib().mml_linearize(self._h, slot, _p(_f64(x)), _p(_f64(T_bl).reshape(16)), w_tan, huber, _p(H), _p(g), C.byref(c)))
        return H, g, c.value

    def linearize_window(self, first, frames, x, T_bl, w_tan=0.0, huber=0.1 / 1.5e-3):
        """Records (frames, 32) of the consecutive slots first .. first + frames - 1 at x (frames, >= 6): one launch."""
        x = _f64(x).reshape(frames, -1)
        rec = np.zeros((frames, NEQ_RECORD_DOUBLES))
        self._ck(lib().mml_linearize_window(self._h, first, frames, x.shape[1], _p(x), _p(_f64(T_bl).reshape(16)), w_tan, huber, _p(rec)))
        return rec

    def linearize_record(self, slot, x, T_bl, d_record_ptr, w_tan=0.0, huber=0.1 / 1.5e-3):
        self._ck(lib().mml_linearize_record(self._h, slot, _p(_f64(x)), _p(_f64(T_bl).reshape(16)), w_tan, huber, C.c_void_p(d_record_ptr)))

    def solve(self, first, count, x, T_bl, window=1, max_iters=10, fixed=False, huber=0.1 / 1.5e-3, w_tan=0.0,
              trace=False):
        x = _f64(x).reshape(count, 6).copy()
        opts = SolveOpts(max_iters, 1 if fixed else 0, huber, w_tan)
        nprob = count // window
        summ = (SolveSummary * nprob)()
        tr = np.zeros((nprob, max_iters, 6 * window)) if trace else None
        self._ck(lib().mml_solve(self._h, first, count, window, _p(_f64(T_bl).reshape(16)), C.byref(opts), _p(x), summ, _p(tr)))
        return x, list(summ), tr

    def estimate(self, first, count, exTlb, P, Q, max_outer=5, inner_iters=10):
        P = _f64(P).reshape(count, 3).copy()
        Q = _f64(Q).reshape(count, 4).copy()
        info = (EstimateInfo * count)()
        self._ck(lib().mml_estimate(self._h, first, count, _p(_f64(exTlb).reshape(16)), _p(P), _p(Q), max_outer, inner_iters, info))
        return P, Q, list(info)

    def step(self, first, count, dR, dt, exTlb, thres_dist, gn_iters, x):
        x = _f64(x).reshape(count, 6).copy()
        self._ck(lib().mml_step(self._h, first, count, _p(_f64(dR).reshape(count, 9)), _p(_f64(dt).reshape(count, 3)), _p(_f64(exTlb).reshape(16)),
                                thres_dist, gn_iters, _p(x)))
        return x

    # ---- multi-GPU (RCCL inside the C-ABI) ----
    def comm_init(self, n_ranks, rank, comm_id):
        r = rccl_libraries()
        if n_ranks > 1 and len(r["loaded"]) > 1:
            raise MmlError(MML_ERR_STATE, "two RCCL copies are mapped into this process (%s): the library and torch.distributed "
                                          "would each drive their own" % ", ".join(r["loaded"]))
        if len(comm_id) != COMM_ID_BYTES:
            raise ValueError("the communicator id is %d bytes" % COMM_ID_BYTES)
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(comm_id))
        self._ck(lib().mml_comm_init(self._h, n_ranks, rank, buf))

    def comm_destroy(self):
        self._ck(lib().mml_comm_destroy(self._h))

    def comm_info(self):
        n, r = C.c_int(0), C.c_int(0)
        self._ck(lib().mml_comm_info(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def window_solve_allgather(self, first, n_local, x_local, T_bl, max_iters=10, fixed=False, huber=0.0, w_tan=3e-4):
        """Joint window solve over n_ranks * n_local frames; returns (own poses, window poses, summary, timing)."""
        n_ranks, _ = self.comm_info()
        x = _f64(x_local).reshape(n_local, 6).copy()
        xw = np.zeros((n_ranks * n_local, 6))
        opts = SolveOpts(max_iters, 1 if fixed else 0, huber, w_tan)
        summ, tim = SolveSummary(), WindowTiming()
        self._ck(lib().mml_window_solve_allgather(self._h, first, n_local, _p(_f64(T_bl).reshape(16)), C.byref(opts), _p(x), _p(xw), C.byref(summ),
                                                  C.byref(tim)))
        return x, xw, summ, tim

    def comm_broadcast_features(self, slot, root):
        self._ck(lib().mml_comm_broadcast_features(self._h, slot, root))

    def comm_broadcast_local_map(self, root):
        self._ck(lib().mml_comm_broadcast_local_map(self._h, root))

    # ---- measurement ----
    def set_lanes(self, lanes):
        self._ck(lib().mml_set_lanes(self._h, lanes))

    def profile_enable(self, on=True):
        self._ck(lib().mml_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        self._ck(lib().mml_profile_reset(self._h))

    def profile_get(self):
        pr = Profile()
        self._ck(lib().mml_profile_get(self._h, C.byref(pr)))
        return {pr.name[i].decode(): (pr.total_ms[i], pr.launches[i]) for i in range(pr.n_stages)}

    def extract_queue_counts(self, slot):
        """(redo, brk): points of the slot's last extraction recomputed with the full decision chain / finished as break-point
        candidates."""
        r, b = C.c_int(0), C.c_int(0)
        self._ck(lib().mml_extract_queue_counts(self._h, slot, C.byref(r), C.byref(b)))
        return r.value, b.value

    def issue_rate(self, kind=0, reps=3):
        """wave64 instructions per second of the device on v_fma_f32 (kind 0) / v_add_u32 (kind 1) chains (mml_issue_rate)."""
        r = C.c_double(0)
        self._ck(lib().mml_issue_rate(self._h, kind, reps, C.byref(r)))
        return r.value

    def libm_f32(self, y, x):
        """(atan2f(y, x), atanf(y)) evaluated by the device's copies of the two libm routines (mml_libm_f32, a test hook)."""
        y, x = np.ascontiguousarray(y, np.float32).ravel(), np.ascontiguousarray(x, np.float32).ravel()
        assert len(x) == len(y)
        o2, o1 = np.empty_like(x), np.empty_like(x)
        self._ck(lib().mml_libm_f32(self._h, _p(y), _p(x), len(x), _p(o2), _p(o1)))
        return o2, o1

    _FIT_SHAPES = {0: (np.float64, 6, np.float64, 12), 1: (np.float64, 15, np.float64, 4), 2: (np.float32, 15, np.float64, 13),
                   3: (np.float32, 18, np.float64, 11), 4: (np.float64, 2, np.float64, 2), 5: (np.float32, 2, np.float32, 2)}

    def model_fit5(self, op, items):
        """The device's line / plane model fit on caller-supplied items (mml_model_fit5, a test hook): op 0 eig3, 1 qr,
        2 line model, 3 plane model, 4 / 5 double / float sqrt and division; layouts in include/mmloam_hip.h."""
        ti, wi, to, wo = self._FIT_SHAPES[op]
        a = np.ascontiguousarray(items, ti).reshape(-1, wi)
        out = np.empty((len(a), wo), to)
        self._ck(lib().mml_model_fit5(self._h, op, _p(a), len(a), _p(out)))
        return out

    def associate_far_count(self):
        """5-NN queries of the last association that went to the far-query kernels (summed over the stream lanes)."""
        n = C.c_int(0)
        self._ck(lib().mml_associate_far_count(self._h, C.byref(n)))
        return n.value

    def device_info(self):
        name = C.create_string_buffer(256)
        cus = C.c_int(0)
        mem = C.c_size_t(0)
        self._ck(lib().mml_device_info(self._h, name, 256, C.byref(cus), C.byref(mem)))
        return name.value.decode(), cus.value, mem.value

    def slot_digest(self, first, count):
        """(count, DIGEST_WORDS) uint64: one digest per slot and piece of state (mml_slot_digest; recomputable on the host from
        the download entry points, see `host_digest`)."""
        out = np.zeros((count, DIGEST_WORDS), np.uint64)
        self._ck(lib().mml_slot_digest(self._h, first, count, _p(out)))
        return out

    def copy_bandwidth(self, nbytes=1 << 30, reps=10):
        g = C.c_double(0)
        self._ck(lib().mml_copy_bandwidth(self._h, nbytes, reps, C.byref(g)))
        return g.value


WIRE_BATCH_MAX = 65535      # MML_WIRE_BATCH_MAX (csrc/wire_decode.h): frames per call of mml_scan_upload_wire_batch


WIRE_TILE_POINTS = 256      # records one workgroup of k_wire_decode_batch takes (csrc/wire_ingest.hip WB_THREADS)


def wire_batch_pack(velo_data, velo_at, n_velo, point_step, offs, livox_data, livox_at, n_livox, livox_record_bytes=19):
    """The arguments of the wire-batch calls as contiguous arrays: (velo bytes or None, velo_at int64 or None, n_velo int32, livox
    bytes or None, livox_at or None, n_livox, (point_step, off_x, off_y, off_z, off_intensity, livox_record_bytes)).  A buffer is
    only checked to reach the last byte its frames announce; every other rule is the library's."""
    def part(data, at, n, rec, m):
        n = np.zeros(m, np.int32) if n is None else np.ascontiguousarray(n, dtype=np.int32).reshape(-1)
        at = None if at is None else np.ascontiguousarray(at, dtype=np.int64).reshape(-1)
        if at is not None and len(at) != len(n):
            raise ValueError("%d offsets for %d counts" % (len(at), len(n)))
        if data is not None:
            data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            if at is not None and len(n) and (n >= 0).all() and (at >= 0).all() and int((at + n.astype(np.int64) * rec)[n > 0].max(initial=0)) > len(data):
                raise ValueError("a payload ends behind the %d bytes of its buffer" % len(data))
            if not len(data):
                data = None
        return data, at, n
    m = len(n_velo) if n_velo is not None else len(n_livox)
    vd, va, nv = part(velo_data, velo_at, n_velo, int(point_step), m)
    ld, la, nl = part(livox_data, livox_at, n_livox, int(livox_record_bytes), m)
    if len(nv) != len(nl):
        raise ValueError("%d Velodyne counts for %d Livox counts" % (len(nv), len(nl)))
    ox, oy, oz, oi = (int(o) for o in offs)
    return vd, va, nv, ld, la, nl, (int(point_step), ox, oy, oz, oi, int(livox_record_bytes))


def scan_upload_wire_plan(velo_at, n_velo, point_step, offs, livox_at, n_livox, livox_record_bytes=19, max_velo_points=-1,
                          max_livox_points=-1):
    """mml_scan_upload_wire_plan: the argument rules of Context.scan_upload_wire_batch alone, on the host.  Returns (rc, span,
    bad_frame): span = [velo first byte, one past velo last byte, livox first, one past livox last] (int64; zeros on a refusal),
    bad_frame = the frame a refusal is about or -1.  A negative capacity is not checked."""
    _, va, nv, _, la, nl, lay = wire_batch_pack(None, velo_at, n_velo, point_step, offs, None, livox_at, n_livox, livox_record_bytes)
    span, bad = np.zeros(4, np.int64), C.c_int(-1)
    rc = lib().mml_scan_upload_wire_plan(len(nv), _p(va), _p(nv), *lay[:5], _p(la), _p(nl), lay[5], max_velo_points, max_livox_points, _p(span),
                                         C.byref(bad))
    return rc, span, bad.value


def wire_decode_host(velo_data, velo_at, n_velo, point_step, offs, livox_data, livox_at, n_livox, livox_record_bytes=19):
    """mml_wire_decode_host: the decode of Context.scan_upload_wire_batch on the host.  Returns (velo (sum n_velo, 4) float32, livox
    (sum n_livox,) LIVOX_DTYPE), frame after frame."""
    vd, va, nv, ld, la, nl, lay = wire_batch_pack(velo_data, velo_at, n_velo, point_step, offs, livox_data, livox_at, n_livox, livox_record_bytes)
    tv, tl = int(np.maximum(nv, 0).sum()), int(np.maximum(nl, 0).sum())
    v, l = np.zeros((max(tv, 1), 4), np.float32), np.zeros(max(tl, 1), LIVOX_DTYPE)
    rc = lib().mml_wire_decode_host(len(nv), _p(vd), _p(va), _p(nv), *lay[:5], _p(ld), _p(la), _p(nl), lay[5], _p(v), _p(l))
    if rc != MML_OK:
        raise MmlError(rc, "mml_wire_decode_host")
    return v[:tv], l[:tl]


def pose_ingest_opts(**over):
    """mml_pose_ingest_opts with the reference's defaults (0.3, 1.5, velo_only_mode 0, first_frame -1), then `over`."""
    o = PoseIngestOpts()
    lib().mml_pose_ingest_opts_default(C.byref(o))
    for k, v in over.items():
        if k not in ("hori_rotate_th", "velo_rotate_th", "velo_only_mode", "first_frame"):
            raise TypeError("unknown ingest option %r" % k)
        setattr(o, k, v)
    return o


def pose_ingest_pack(clouds, n_points=None, rows=None, opts=None):
    """The arguments of mml_pose_ingest_batch from what the wrappers hand out: (block uint8, n_points (n, 6) int32, rows or
    None, PoseIngestOpts).  A list of six-array tuples is concatenated into the block; a block is taken as it is."""
    if n_points is None:
        msgs = [tuple(np.ascontiguousarray(c).view(np.uint8).reshape(-1, 48) for c in six) for six in clouds]
        if any(len(six) != 6 for six in msgs):
            raise ValueError("a message is six clouds (FEATURE_CLOUD_NAMES)")
        n = np.array([[len(c) for c in six] for six in msgs], np.int32).reshape(-1, 6)
        parts = [c for six in msgs for c in six if len(c)]
        block = np.concatenate(parts) if parts else np.zeros((0, 48), np.uint8)
    else:
        n = np.ascontiguousarray(n_points, dtype=np.int32).reshape(-1, 6)
        block = np.ascontiguousarray(clouds).view(np.uint8).reshape(-1) if clouds is not None else np.zeros(0, np.uint8)
        if clouds is not None and (n >= 0).all() and block.size != 48 * int(n.sum()):
            raise ValueError("the block holds %d bytes, n_points announces %d records" % (block.size, int(n.sum())))
    r = None
    if rows is not None:
        r = np.ascontiguousarray(rows, dtype=IMU_INTERVAL_DTYPE).reshape(-1)
        if len(r) != len(n):
            raise ValueError("%d fetch rows for %d messages" % (len(r), len(n)))
    return np.ascontiguousarray(block), n, r, pose_ingest_opts(**(opts or {}))


def pose_ingest_plan(n_points, rows=None, **opts):
    """mml_pose_ingest_plan: the decisions of Context.pose_ingest alone, on the host (the same routine).  n_points (n, 6)."""
    _, n, r, o = pose_ingest_pack(None, n_points, rows, opts)
    out = np.zeros(max(len(n), 1), POSE_INGEST_ROW_DTYPE)
    rc = lib().mml_pose_ingest_plan(len(n), _p(n), _p(r), C.byref(o), _p(out))
    if rc != MML_OK:
        raise MmlError(rc, "mml_pose_ingest_plan")
    return out[:len(n)]


class ImuPreint(C.Structure):
    _fields_ = [("dp", C.c_double * 3), ("dv", C.c_double * 3), ("dq", C.c_double * 4), ("dtime", C.c_double),
                ("bg", C.c_double * 3), ("ba", C.c_double * 3), ("jacobian", C.c_double * 225),
                ("covariance", C.c_double * 225)]


class Prior(C.Structure):
    _fields_ = [("J", C.c_double * 225), ("r0", C.c_double * 15), ("x0", C.c_double * 15)]


def imu_preintegrate(samples, bg, ba):
    """IMUIntegrator::PreIntegration: samples (n, 7) = gyro xyz, accel xyz (message units), dt."""
    smp = _f64(samples).reshape(-1, 7)
    out = ImuPreint()
    rc = lib().mml_imu_preintegrate(_p(smp), len(smp), _p(_f64(bg)), _p(_f64(ba)), C.byref(out))
    if rc != MML_OK:
        raise MmlError(rc, "mml_imu_preintegrate")
    return out


def imu_preintegrate_batch(samples_list, bg, ba, ctx=None):
    """mml_imu_preintegrate_batch: imu_preintegrate for a list of intervals in one call.  samples_list[i]: (k_i, 7), k_i >= 0;
    bg, ba: one vector for all intervals or one per interval (n, 3).  ctx None: the host routine (no device needed); a
    Context: one upload, one launch, one read-back, bit-identical to it.  Returns a list of ImuPreint."""
    n = len(samples_list)
    smp = [_f64(s).reshape(-1, 7) for s in samples_list]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in smp])]).astype(np.int32)
    flat = _f64(np.concatenate(smp)) if offsets[-1] else np.zeros((1, 7))
    bias = []
    for name, b in (("bg", bg), ("ba", ba)):
        b = np.asarray(b, dtype=np.float64)
        if b.shape not in ((3,), (n, 3)):
            raise ValueError("%s must be one vector or one per interval (%d, 3), not %s" % (name, n, b.shape))
        bias.append(np.ascontiguousarray(np.broadcast_to(b, (n, 3))))
    out = (ImuPreint * max(n, 1))()
    rc = lib().mml_imu_preintegrate_batch(ctx._h if ctx is not None else None, n, _p(flat), _p(offsets), _p(bias[0]), _p(bias[1]), out)
    if ctx is not None:
        ctx._ck(rc)
    elif rc != MML_OK:
        raise MmlError(rc, "mml_imu_preintegrate_batch")
    return [ImuPreint.from_buffer_copy(out[i]) for i in range(n)]


def imu_fetch_raw(stream_or_msgs, t_start, t_end, bg=None, ba=None, ctx=None, want=("samples", "pre", "dq"), sample_capacity=None):
    """mml_imu_fetch_batch (an ImuStream) / mml_imu_fetch_host (an (m, 7) array of messages) without the error check: returns
    (rc, out) with out = dict(rows (IMU_INTERVAL_DTYPE), offsets (n + 1), and -- as far as `want` names them -- samples
    (offsets[n], 7), pre (a ctypes array of n ImuPreint), dq (n, 4)).  sample_capacity None: the rows are counted by a sizing
    call first (one more synchronisation on a stream); give a bound to save it.  After MML_ERR_CAPACITY rows and offsets are
    valid and the rest is not; after any other refusal nothing is.  Without biases `pre` is left out."""
    ts, te = _f64(t_start).reshape(-1), _f64(t_end).reshape(-1)
    n = len(ts)
    if len(te) != n:
        raise ValueError("t_start and t_end differ in length (%d, %d)" % (n, len(te)))
    unknown = set(want) - {"samples", "pre", "dq"}
    if unknown:
        raise ValueError("want names %s" % sorted(unknown))
    if bg is None and ba is None:
        want = tuple(w for w in want if w != "pre")     # (no biases: no pre-integration)
    bias = [None, None]
    if bg is not None or ba is not None:
        for k, (name, b) in enumerate((("bg", bg), ("ba", ba))):
            if b is None:
                continue
            b = np.asarray(b, dtype=np.float64)
            if b.shape not in ((3,), (n, 3)):
                raise ValueError("%s must be one vector or one per interval (%d, 3), not %s" % (name, n, b.shape))
            bias[k] = np.ascontiguousarray(np.broadcast_to(b, (n, 3)))
    rows = np.zeros(max(n, 1), IMU_INTERVAL_DTYPE)
    offsets = np.zeros(n + 1, np.int32)
    if isinstance(stream_or_msgs, ImuStream):
        ctx = stream_or_msgs._ctx if ctx is None else ctx

        def call(smp, cap, pre, dq):
            return lib().mml_imu_fetch_batch(ctx._h, stream_or_msgs._h, n, _p(ts), _p(te), _p(bias[0]), _p(bias[1]), _p(rows), _p(offsets), _p(smp),
                                             cap, pre, _p(dq))
    else:
        msgs = _f64(stream_or_msgs).reshape(-1, 7)

        def call(smp, cap, pre, dq):
            return lib().mml_imu_fetch_host(_p(msgs) if len(msgs) else None, len(msgs), n, _p(ts), _p(te), _p(bias[0]), _p(bias[1]), _p(rows),
                                            _p(offsets), _p(smp), cap, pre, _p(dq))
    out = dict(rows=rows[:n], offsets=offsets)
    if not want:
        return call(None, 0, None, None), out
    if sample_capacity is None:
        rc = call(None, 0, None, None)
        if rc != MML_OK:
            return rc, out
        sample_capacity = int(offsets[n])
    smp = np.zeros((max(int(sample_capacity), 1), 7)) if "samples" in want else None
    pre = (ImuPreint * max(n, 1))() if "pre" in want else None
    dq = np.zeros((max(n, 1), 4)) if "dq" in want else None
    rc = call(smp, int(sample_capacity), pre, dq)
    if rc == MML_OK:
        if smp is not None:
            out["samples"] = smp[:int(offsets[n])]
        if pre is not None:
            out["pre"] = pre
        if dq is not None:
            out["dq"] = dq[:n]
    return rc, out


def imu_fetch_batch(stream_or_msgs, t_start, t_end, bg=None, ba=None, ctx=None, want=("samples", "pre", "dq"), sample_capacity=None):
    """fetchImuMsgs for n intervals (t_start[i], t_end[i]] in one call, with the pre-integration (bg, ba: one vector or one per
    interval) and the gyro integration of what it cuts: imu_fetch_raw with the error check.  An ImuStream: the device call;
    an (m, 7) array of messages: the host routine, bit-identical to it."""
    rc, out = imu_fetch_raw(stream_or_msgs, t_start, t_end, bg, ba, ctx, want, sample_capacity)
    if rc != MML_OK:
        if isinstance(stream_or_msgs, ImuStream):
            stream_or_msgs._ctx._ck(rc)
        raise MmlError(rc, "mml_imu_fetch_host")
    return out


def imu_predict_batch(exTlb, prev=None, pre=None, dq=None, ctx=None):
    """mml_imu_predict_batch: the frame prediction of the pose node for n intervals.  prev (n, 10: P, Q x y z w, V of the
    previous frame) with pre (n ImuPreint, list or ctypes array): state (n, 10), delta_Rl (n, 3, 3), delta_tl (n, 3) -- the dR /
    dt of Context.step / undistort; dq (n, 4): gyro_Rb, gyro_Rl (n, 3, 3), the bring-up branch.  ctx None: the host routine."""
    ex = _f64(exTlb).reshape(4, 4)
    out = {}
    n = len(prev) if prev is not None else len(dq)
    args = [None] * 5
    if prev is not None:
        pv = _f64(prev).reshape(n, 10)
        arr = pre if isinstance(pre, C.Array) else (ImuPreint * n)(*pre)
        out.update(state=np.zeros((n, 10)), delta_Rl=np.zeros((n, 3, 3)), delta_tl=np.zeros((n, 3)))
        args = [_p(pv), arr, _p(out["state"]), _p(out["delta_Rl"]), _p(out["delta_tl"])]
    gargs = [None] * 3
    if dq is not None:
        q = _f64(dq).reshape(n, 4)
        out.update(gyro_Rb=np.zeros((n, 3, 3)), gyro_Rl=np.zeros((n, 3, 3)))
        gargs = [_p(q), _p(out["gyro_Rb"]), _p(out["gyro_Rl"])]
    rc = lib().mml_imu_predict_batch(ctx._h if ctx is not None else None, n, _p(ex), *(args + gargs))
    if ctx is not None:
        ctx._ck(rc)
    elif rc != MML_OK:
        raise MmlError(rc, "mml_imu_predict_batch")
    return out


def imu_factor(pre, gravity, pr_i, vb_i, pr_j, vb_j, jac=True):
    """Cost_NavState_PRV_Bias: weighted residual (15) and Jacobian (15, 30) [pr_i | vb_i | pr_j | vb_j]."""
    r = np.zeros(15)
    J = np.zeros((15, 30)) if jac else None
    rc = lib().mml_imu_factor(C.byref(pre), _p(_f64(gravity)), _p(_f64(pr_i)), _p(_f64(vb_i)), _p(_f64(pr_j)),
                              _p(_f64(vb_j)), _p(r), _p(J))
    if rc != MML_OK:
        raise MmlError(rc, "mml_imu_factor")
    return r, J


class LioInitResult(C.Structure):
    _fields_ = [("status", C.c_int), ("fail_frame", C.c_int), ("keep_from", C.c_int), ("_pad", C.c_int),
                ("gravity", C.c_double * 3), ("r_wg", C.c_double * 3), ("q_wg", C.c_double * 4),
                ("average_acc", C.c_double * 3), ("ba", C.c_double * 3), ("bg", C.c_double * 3),
                ("gravity_solve", SolveSummary), ("joint_solve", SolveSummary)]


LIO_INIT_OK, LIO_INIT_BIAS, LIO_INIT_VELOCITY = 0, 1, 2
LIO_INIT_NOT_PD = 3  # mml_lio_initialize_batch only: a pre-integration covariance is not positive definite (nothing written)


def imu_gyro_integrate(samples, dq=(0.0, 0.0, 0.0, 1.0)):
    """IMUIntegrator::GyroIntegration: the gyro samples (n, 7) accumulated onto dq (x, y, z, w).  Returns the new dq."""
    smp = _f64(samples).reshape(-1, 7)
    q = _f64(dq).reshape(4).copy()
    rc = lib().mml_imu_gyro_integrate(_p(smp), len(smp), _p(q))
    if rc != MML_OK:
        raise MmlError(rc, "mml_imu_gyro_integrate")
    return q


def imu_init_factor(pre, ri, rj, dp, rwg, vi, vj, ba, bg, jac=True):
    """Cost_Initialization_IMU: weighted residual (9) and Jacobian (9, 15) [rwg | vi | vj | ba | bg]."""
    r = np.zeros(9)
    J = np.zeros((9, 15)) if jac else None
    rc = lib().mml_imu_init_factor(C.byref(pre), *[_p(_f64(a).reshape(3)) for a in (ri, rj, dp, rwg, vi, vj, ba, bg)],
                                   _p(r), _p(J))
    if rc != MML_OK:
        raise MmlError(rc, "mml_imu_init_factor")
    return r, J


def lio_initialize(t, P, Q, V, bg, ba, samples, exTlb, pre=None):
    """TryMAPInitialization on arrays (mml_lio_initialize).  t (n,), P (n,3), Q (n,4 x y z w), V / bg / ba (n,3); samples:
    a list of n (k_i, 7) arrays (frame i's IMU messages); pre: None or a list of n pre-integrations (entry 0 unused).
    Returns (result, dict of the written P, Q, V, bg, ba arrays, list of n pre-integrations with entry 0 None)."""
    n = len(t)
    st = {k: _f64(a).reshape(n, w).copy() for k, a, w in (("P", P, 3), ("Q", Q, 4), ("V", V, 3), ("bg", bg, 3), ("ba", ba, 3))}
    smp = [_f64(s).reshape(-1, 7) for s in samples]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in smp])]).astype(np.int32)
    flat = _f64(np.concatenate(smp) if offsets[-1] else np.zeros((0, 7)))
    pin = None
    if pre is not None:
        pin = (ImuPreint * n)()
        for i in range(1, n):
            pin[i] = pre[i]
    pout = (ImuPreint * n)()
    res = LioInitResult()
    rc = lib().mml_lio_initialize(n, _p(_f64(t).reshape(n)), _p(st["P"]), _p(st["Q"]), _p(st["V"]), _p(st["bg"]), _p(st["ba"]), _p(flat), _p(offsets),
                                  _p(_f64(exTlb).reshape(16)), pin, pout, C.byref(res))
    if rc != MML_OK:
        raise MmlError(rc, "mml_lio_initialize")
    pres = [None] + [ImuPreint.from_buffer_copy(pout[i]) for i in range(1, n)]
    return res, st, pres


def lio_initialize_batch(segments, ctx=None):
    """mml_lio_initialize_batch: lio_initialize for a list of segments in one call.  segments[s]: the arguments of lio_initialize
    as a tuple (t, P, Q, V, bg, ba, samples, exTlb[, pre]).  The C call takes pre-integrations for all segments or for none: when
    some segments bring theirs, the others' are made first by imu_preintegrate_batch (the routine the call itself would use, at
    frame i-1's biases).  ctx None: the host routine (no device needed); a Context: one upload, three launches, one read-back,
    bit-identical to it.  Returns per segment what lio_initialize returns: (result, dict of the written P, Q, V, bg, ba, list of
    n pre-integrations with entry 0 None); a segment with status LIO_INIT_NOT_PD has its state as it came in and no
    pre-integrations (all None)."""
    n_seg = len(segments)
    segs = [tuple(s) + (None,) * (9 - len(s)) for s in segments]
    ns = [len(s[0]) for s in segs]
    fo = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    F = int(fo[-1])
    widths = (("P", 1, 3), ("Q", 2, 4), ("V", 3, 3), ("bg", 4, 3), ("ba", 5, 3))
    st = {k: (np.concatenate([_f64(s[j]).reshape(n, w) for s, n in zip(segs, ns)]) if F else np.zeros((0, w))) for k, j, w in widths}
    t = _f64(np.concatenate([_f64(s[0]).reshape(n) for s, n in zip(segs, ns)])) if F else np.zeros(0)
    smp = [[_f64(a).reshape(-1, 7) for a in s[6]] for s in segs]
    for s, (m, n) in enumerate(zip(smp, ns)):
        if len(m) != n:
            raise ValueError("segment %d: %d frames but %d sample arrays" % (s, n, len(m)))
    so = np.concatenate([[0], np.cumsum([len(a) for m in smp for a in m])]).astype(np.int32)
    flat = _f64(np.concatenate([a for m in smp for a in m])) if so[-1] else np.zeros((1, 7))
    ex = _f64(np.stack([_f64(s[7]).reshape(16) for s in segs])) if n_seg else np.zeros((1, 16))
    pin = None
    if any(s[8] is not None for s in segs):
        pin = (ImuPreint * max(F, 1))()
        todo = [(s, i) for s in range(n_seg) if segs[s][8] is None for i in range(1, ns[s])]
        made = iter(imu_preintegrate_batch([smp[s][i] for s, i in todo], np.stack([st["bg"][fo[s] + i - 1] for s, i in todo]),
                                           np.stack([st["ba"][fo[s] + i - 1] for s, i in todo]), ctx) if todo else [])
        for s in range(n_seg):
            for i in range(1, ns[s]):
                pin[fo[s] + i] = segs[s][8][i] if segs[s][8] is not None else next(made)
    pout = (ImuPreint * max(F, 1))()
    res = (LioInitResult * max(n_seg, 1))()
    rc = lib().mml_lio_initialize_batch(ctx._h if ctx is not None else None, n_seg, _p(fo), _p(t), _p(st["P"]), _p(st["Q"]), _p(st["V"]),
                                        _p(st["bg"]), _p(st["ba"]), _p(flat), _p(so), _p(ex), pin, pout, res)
    if ctx is not None:
        ctx._ck(rc)
    elif rc != MML_OK:
        raise MmlError(rc, "mml_lio_initialize_batch")
    ret = []
    for s in range(n_seg):
        a, b = int(fo[s]), int(fo[s + 1])
        r = LioInitResult.from_buffer_copy(res[s])
        pres = [None] + [ImuPreint.from_buffer_copy(pout[f]) if r.status != LIO_INIT_NOT_PD else None for f in range(a + 1, b)]
        ret.append((r, {k: v[a:b].copy() for k, v in st.items()}, pres))
    return ret


class FullWindowSolver:
    """Estimator::Estimate in full-window mode on the host: W x [PR 6 | VBias 9], lidar records from the device,
    IMU factors between consecutive frames, optional marginalization prior on frame 0."""

    def __init__(self, W, max_iters=10, fixed=False, huber=0.0, w_tan=3e-4):
        self.W = W
        self._opts = SolveOpts(max_iters, 1 if fixed else 0, huber, w_tan)
        self._h = C.c_void_p(lib().mml_fullwindow_create(W, C.byref(self._opts)))
        if not self._h:
            raise MmlError(MML_ERR_INVALID, "mml_fullwindow_create failed")

    def _ck(self, rc, what):
        if rc < 0:
            raise MmlError(rc, what)
        return rc

    def set_imu(self, f, pre, gravity):
        self._ck(lib().mml_fullwindow_set_imu(self._h, f, C.byref(pre), _p(_f64(gravity))), "set_imu")

    def set_prior(self, prior):
        self._ck(lib().mml_fullwindow_set_prior(self._h, C.byref(prior) if prior is not None else None), "set_prior")

    def step(self, records, x_eval):
        rec = _f64(records).reshape(self.W, NEQ_RECORD_DOUBLES)
        x = _f64(x_eval).reshape(self.W, 15).copy()
        rc = self._ck(lib().mml_fullwindow_step(self._h, _p(rec), _p(x)), "mml_fullwindow_step")
        return rc == 1, x

    def solve_device(self, ctx, first_slot, T_bl, x):
        """mml_fullwindow_solve: the whole trust-region loop on the device (frames in consecutive, associated slots).
        Returns (x, summary, evaluations)."""
        x = _f64(x).reshape(self.W, 15).copy()
        T = _f64(T_bl).reshape(16)
        s = SolveSummary()
        ev = C.c_int(0)
        ctx._ck(lib().mml_fullwindow_solve(ctx._h, self._h, first_slot, _p(T), _p(x), C.byref(s), C.byref(ev)))
        return x, s, ev.value

    def summary(self):
        s = SolveSummary()
        lib().mml_fullwindow_summary(self._h, C.byref(s))
        return s

    def normal_equations(self, records, x):
        n = 15 * self.W
        H = np.zeros((n, n))
        g = np.zeros(n)
        c = C.c_double(0)
        self._ck(lib().mml_fullwindow_normal_equations(self._h, _p(_f64(records).reshape(self.W, NEQ_RECORD_DOUBLES)),
                                                       _p(_f64(x).reshape(self.W, 15)), _p(H), _p(g), C.byref(c)), "normal_equations")
        return H, g, c.value

    def marginalize(self, lidar_record0, x):
        out = Prior()
        self._ck(lib().mml_fullwindow_marginalize(self._h, _p(_f64(lidar_record0).reshape(NEQ_RECORD_DOUBLES)),
                                                  _p(_f64(x).reshape(self.W, 15)), C.byref(out)), "marginalize")
        return out

    def marginalize_device(self, ctx, first_slot, T_bl, x):
        """mml_fullwindow_marginalize_batch for this window alone: the prior `marginalize` returns for the loss-free record
        of slot `first_slot` at x[0], computed on the device without fetching that record."""
        return fullwindow_marginalize_batch(ctx, [self], [first_slot], T_bl, [x])[0]

    def __del__(self):
        try:
            if self._h:
                lib().mml_fullwindow_destroy(self._h)
                self._h = None
        except Exception:
            pass


def fullwindow_solve_batch(ctx, solvers, first_slots, T_bl, xs, records0=False):
    """mml_fullwindow_solve_batch: the device-resident solve of FullWindowSolver.solve_device for a list of windows in one
    device call.  solvers[w]: the FullWindowSolver of window w (its own W, options, IMU factors, prior), first_slots[w]: its
    first scan slot, xs[w]: its state (W_w, 15).  Returns (list of x (W_w, 15), list of SolveSummary, list of evaluation
    counts) and, with records0=True, a fourth entry: the (n, 32) records of every window's frame 0 at the returned x (what
    FullWindowSolver.marginalize takes).  Every window's result equals solve_device called on it alone."""
    n = len(solvers)
    if len(first_slots) != n or len(xs) != n:
        raise ValueError("solvers, first_slots and xs must have one entry per window (%d, %d, %d)" % (n, len(first_slots), len(xs)))
    x = np.zeros((max(n, 1), FW_X_STRIDE))
    for w, (fw, xw) in enumerate(zip(solvers, xs)):
        xw = np.asarray(xw, dtype=np.float64)
        if xw.shape != (fw.W, 15):
            raise ValueError("xs[%d] has shape %s, window %d needs (%d, 15)" % (w, xw.shape, w, fw.W))
        x[w, :15 * fw.W] = xw.reshape(-1)
    handles = (C.c_void_p * max(n, 1))(*[fw._h.value if isinstance(fw._h, C.c_void_p) else fw._h for fw in solvers])
    first = np.ascontiguousarray(list(first_slots) + [0] * (n == 0), dtype=np.int32)
    summ = (SolveSummary * max(n, 1))()
    ev = np.zeros(max(n, 1), np.int32)
    rec = np.zeros((max(n, 1), NEQ_RECORD_DOUBLES)) if records0 else None
    ctx._ck(lib().mml_fullwindow_solve_batch(ctx._h, n, handles, _p(first), _p(_f64(T_bl).reshape(16)), _p(x), summ, _p(ev), _p(rec)))
    out = ([x[w, :15 * fw.W].reshape(fw.W, 15).copy() for w, fw in enumerate(solvers)], list(summ)[:n], [int(e) for e in ev[:n]])
    return out + (rec[:n],) if records0 else out


def fullwindow_marginalize_batch(ctx, solvers, first_slots, T_bl, xs):
    """mml_fullwindow_marginalize_batch: FullWindowSolver.marginalize for a list of windows in one device call.  solvers[w]:
    the FullWindowSolver of window w (W >= 2, IMU factor 1 set; a solver may appear more than once), first_slots[w]: the
    scan slot of its frame 0, xs[w]: its state (W_w, 15).  Returns a list of Prior, each bit-identical to
    solvers[w].marginalize(record, xs[w]) with the loss-free record of that slot at xs[w][0]."""
    n = len(solvers)
    if len(first_slots) != n or len(xs) != n:
        raise ValueError("solvers, first_slots and xs must have one entry per window (%d, %d, %d)" % (n, len(first_slots), len(xs)))
    x = np.zeros((max(n, 1), FW_X_STRIDE))
    for w, (fw, xw) in enumerate(zip(solvers, xs)):
        xw = np.asarray(xw, dtype=np.float64)
        if xw.shape != (fw.W, 15):
            raise ValueError("xs[%d] has shape %s, window %d needs (%d, 15)" % (w, xw.shape, w, fw.W))
        x[w, :15 * fw.W] = xw.reshape(-1)
    handles = (C.c_void_p * max(n, 1))(*[fw._h.value if isinstance(fw._h, C.c_void_p) else fw._h for fw in solvers])
    first = np.ascontiguousarray(list(first_slots) + [0] * (n == 0), dtype=np.int32)
    out = (Prior * max(n, 1))()
    rc = lib().mml_fullwindow_marginalize_batch(ctx._h if ctx is not None else None, n, handles, _p(first), _p(_f64(T_bl).reshape(16)), _p(x), out)
    if ctx is not None:
        ctx._ck(rc)
    elif rc != MML_OK:
        raise MmlError(rc, "mml_fullwindow_marginalize_batch")
    return [Prior.from_buffer_copy(out[w]) for w in range(n)]


def marginalize_dense(ctx, A, b):
    """The dense tail of the marginalization on caller-supplied systems (mml_marginalize_dense, a test hook).  A: (n, 30, 30)
    or (30, 30), the first 15 parameters are marginalized; b: (n, 30) or (30,).  ctx None: the host routine (no device
    needed); a Context: the device routine, bit-identical to it.  Returns (J (n, 15, 15), r0 (n, 15)), without the leading
    axis for a single system."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    single = A.ndim == 2
    if A.shape[-2:] != (30, 30) or A.ndim not in (2, 3):
        raise ValueError("A must be (n, 30, 30) or (30, 30), not %s" % (A.shape,))
    if b.shape != A.shape[:-2] + (30,):
        raise ValueError("b must be %s, not %s" % (A.shape[:-2] + (30,), b.shape))
    A = np.ascontiguousarray(A.reshape(-1, 900))
    b = np.ascontiguousarray(b.reshape(-1, 30))
    n = len(A)
    J, r0 = np.zeros((n, 15, 15)), np.zeros((n, 15))
    rc = lib().mml_marginalize_dense(ctx._h if ctx is not None else None, n, _p(A), _p(b), _p(J), _p(r0))
    if ctx is not None:
        ctx._ck(rc)
    elif rc != MML_OK:
        raise MmlError(rc, "mml_marginalize_dense")
    return (J[0], r0[0]) if single else (J, r0)


TR_DIGEST_DOUBLES, TR_DIGEST_INTS = 56, 16
TR_DIGEST_FIELDS = ("cost", "radius", "mu", "alpha", "dogleg_norm", "model_change", "step_norm", "x_norm")
TR_DIGEST_INT_FIELDS = ("iter", "successful", "num_invalid", "reuse", "termination", "go", "evaluate", "decide", "nprop")


def tr_replay(ctx, variant, scripts):
    """The trust-region state machine replayed on records given in advance (mml_debug_tr_replay, a test hook).  scripts: a list of
    dicts with W, fixed, max_iters, x0 (6 W) and records (R, W, 28); variant 0 is the host's tr_propose / tr_decide (ctx may be
    None), 1..4 the device copies (include/mmloam_hip.h).  Returns (xc (N, Rmax, 48), digest (N, Rmax, 56), digest_i (N, Rmax, 16));
    the rounds of a script beyond its own R stay zero."""
    n = len(scripts)
    rmax = max([np.asarray(s["records"]).shape[0] for s in scripts] + [1])
    hdr = np.zeros((n, 4), np.int32)
    x0 = np.zeros((n, 48))
    rec = np.zeros((n, rmax, 8, 28))
    for k, s in enumerate(scripts):
        r = np.asarray(s["records"], dtype=np.float64)
        W = int(s["W"])
        if r.ndim != 3 or r.shape[1:] != (W, 28):
            raise ValueError("script %d: records must be (R, %d, 28), not %s" % (k, W, r.shape))
        hdr[k] = (W, int(s["fixed"]), int(s["max_iters"]), r.shape[0])
        x0[k, :6 * W] = np.asarray(s["x0"], dtype=np.float64).reshape(6 * W)
        rec[k, :r.shape[0], :W] = r
    xc, dig = np.zeros((n, rmax, 48)), np.zeros((n, rmax, TR_DIGEST_DOUBLES))
    digi = np.zeros((n, rmax, TR_DIGEST_INTS), np.int32)
    rc = lib().mml_debug_tr_replay(ctx._h if ctx is not None else None, variant, n, rmax, _p(hdr), _p(x0), _p(rec), _p(xc), _p(dig), _p(digi))
    if ctx is not None:
        ctx._ck(rc)
    elif rc != MML_OK:
        raise MmlError(rc, "mml_debug_tr_replay")
    return xc, dig, digi


PHASE_CLOCKS_UNKNOWN, PHASE_CLOCKS_NOT_BUILT = -1, -2


def phase_clocks(family, out, reset=False):
    """mml_debug_phase_clocks (a test hook; csrc/phase_clock.h, tools/phases.py): the slots of a timing build's phase clocks into the
    ctypes c_ulonglong array out, or all of them zeroed.  Returns the slot count or a negative code (the two above; -3 out too small; -4 HIP)."""
    return lib().mml_debug_phase_clocks(family.encode(), out, len(out), int(reset))


FW_DIGEST_DOUBLES = 128


def fw_replay(ctx, variant, scripts):
    """The full-window trust-region state machine replayed on normal equations given in advance (mml_debug_fw_replay, a test hook).
    scripts: a list of dicts with W, fixed, max_iters, x0 (15 W) and records, a list of R rounds (band (15 W, 45), g (15 W), cost);
    variant 0 is the host's propose / decide (ctx may be None), 1 the device's fw_round.  The rounds go over packed raggedly.
    Returns (xc (N, Rmax, 120), digest (N, Rmax, 128), digest_i (N, Rmax, 16)); the rounds of a script beyond its own R stay zero."""
    n = len(scripts)
    hdr = np.zeros((n, 4), np.int32)
    x0 = np.zeros((max(n, 1), 120))
    off = np.zeros(max(n, 1), np.int64)
    parts, pos = [], 0
    for k, s in enumerate(scripts):
        W = int(s["W"])
        m = 15 * W
        hdr[k] = (W, int(s["fixed"]), int(s["max_iters"]), len(s["records"]))
        x0[k, :m] = np.asarray(s["x0"], dtype=np.float64).reshape(m)
        off[k] = pos
        for r, (band, g, cost) in enumerate(s["records"]):
            band, g = np.asarray(band, dtype=np.float64), np.asarray(g, dtype=np.float64)
            if band.shape != (m, 45) or g.shape != (m,):
                raise ValueError("script %d round %d: band must be (%d, 45) and g (%d,), not %s and %s" % (k, r, m, m, band.shape, g.shape))
            parts += [band.reshape(-1), g, np.array([cost], dtype=np.float64)]
            pos += 46 * m + 1
    rounds = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(1)
    rows = int(hdr[:, 3].sum())
    xc, dig = np.zeros((max(rows, 1), 120)), np.zeros((max(rows, 1), FW_DIGEST_DOUBLES))
    digi = np.zeros((max(rows, 1), TR_DIGEST_INTS), np.int32)
    rc = lib().mml_debug_fw_replay(ctx._h if ctx is not None else None, variant, n, _p(hdr), _p(x0), _p(off), _p(rounds), pos, _p(xc), _p(dig),
                                   _p(digi))
    if ctx is not None:
        ctx._ck(rc)
    elif rc != MML_OK:
        raise MmlError(rc, "mml_debug_fw_replay")
    rmax = int(hdr[:, 3].max()) if n else 1
    XC, DG, DI = np.zeros((n, rmax, 120)), np.zeros((n, rmax, FW_DIGEST_DOUBLES)), np.zeros((n, rmax, TR_DIGEST_INTS), np.int32)
    row = 0
    for k in range(n):
        R = int(hdr[k, 3])
        XC[k, :R], DG[k, :R], DI[k, :R] = xc[row:row + R], dig[row:row + R], digi[row:row + R]
        row += R
    return XC, DG, DI


class WindowSolver:
    """Host-side joint dogleg over W all-gathered 32-double records; needs no device."""

    def __init__(self, W, max_iters=10, fixed=False, huber=0.0, w_tan=3e-4):
        self.W = W
        self._opts = SolveOpts(max_iters, 1 if fixed else 0, huber, w_tan)
        self._h = lib().mml_window_solver_create(W, C.byref(self._opts))
        if not self._h:
            raise MmlError(MML_ERR_INVALID, "mml_window_solver_create failed")

    def step(self, records, x_eval):
        """records: (W,32) at x_eval (W,6).  Returns (done, next x_eval)."""
        rec = _f64(records).reshape(self.W, NEQ_RECORD_DOUBLES)
        x = _f64(x_eval).reshape(self.W, 6).copy()
        rc = lib().mml_window_solver_step(self._h, _p(rec), _p(x))
        if rc < 0:
            raise MmlError(rc, "mml_window_solver_step")
        return rc == 1, x

    def summary(self):
        s = SolveSummary()
        lib().mml_window_solver_summary(self._h, C.byref(s))
        return s

    def __del__(self):
        try:
            if self._h:
                lib().mml_window_solver_destroy(self._h)
                self._h = None
        except Exception:
            pass


def pack_record(H, g, cost, n_line_used=0, n_plane_used=0):
    """(6x6 H, g, cost) -> the 32-double all-gather record of include/mmloam_hip.h."""
    rec = np.zeros(NEQ_RECORD_DOUBLES)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            rec[k] = H[a, b]
            k += 1
    rec[21:27] = g
    rec[27] = cost
    rec[28] = n_line_used
    rec[29] = n_plane_used
    return rec


# every struct of include/mmloam_hip.h that the package mirrors -> its ctypes.Structure, its numpy dtype, or both
# (tests/test_abi_structs.py compiles the header and holds each mirror's size and field offsets against the C compiler's)
ABI_STRUCTS = {
    "mml_livox_point": LIVOX_DTYPE, "mml_config": Config, "mml_world_map_info": WorldMapInfo, "mml_velo_fov_info": VELO_FOV_INFO_DTYPE,
    "mml_livox_stream_state": LivoxStreamState, "mml_union_frame": UNION_FRAME_DTYPE, "mml_time_offset_estimate_row": TOFS_ROW_DTYPE,
    "mml_gicp_info": GicpInfo, "mml_gicp_opts": GicpOpts, "mml_calib_info": CalibInfo, "mml_scan_info": ScanInfo,
    "mml_assoc_stats": AssocStats, "mml_solve_opts": SolveOpts, "mml_solve_summary": SolveSummary, "mml_estimate_info": EstimateInfo,
    "mml_wm_assoc_opts": WmAssocOpts, "mml_wm_localize_opts": WmLocalizeOpts, "mml_wm_score": (WmScore, WM_SCORE_DT),
    "mml_wm_score_opts": WmScoreOpts, "mml_wm_reloc_opts": WmRelocOpts, "mml_wm_reloc_info": WmRelocInfo,
    "mml_wm_evict_rule": WmEvictRule, "mml_wm_evict_info": WmEvictInfo,
    "mml_window_timing": WindowTiming, "mml_profile": Profile, "mml_imu_preint": ImuPreint, "mml_prior": Prior,
    "mml_lio_init_result": LioInitResult, "mml_imu_stream_state": ImuStreamState, "mml_imu_interval": IMU_INTERVAL_DTYPE,
    "mml_pose_ingest_opts": PoseIngestOpts, "mml_pose_ingest_row": POSE_INGEST_ROW_DTYPE, "mml_gicp_debug": GicpDebug,
}
