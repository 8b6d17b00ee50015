// pose_ingest.h -- what the pose node does with a union_cloud message before the first RemoveLidarDistortion
// (unionPoseEstimation.cpp:719-773), as ONE host routine: mml_pose_ingest_plan and mml_pose_ingest_batch both run
// pose_ingest_plan() below, so the device call cannot decide differently from the plan.  Host code only, no HIP: a program
// without kernels can include it.
//
// `abs` in the reference is the unqualified call on a double (angular_velocity.z is float64 in sensor_msgs/Imu).  The TU includes
// Estimator/Estimator.h (:32) -> <tf/tf.h> (Estimator.h:12) -> tf/LinearMath/Scalar.h -> <math.h>, and libstdc++'s <math.h>
// (gcc >= 6; melodic: 7.5) adds `using std::abs;` to the global namespace: overload resolution takes std::abs(double), not the C
// library's abs(int) that <cstdlib> alone would leave (which truncates 0.9 to 0).  DESIGN.md section 2, convention 14;
// tests/test_pose_ingest_host.py compiles both cases.
#ifndef MML_POSE_INGEST_H
#define MML_POSE_INGEST_H

#include <limits.h>
#include <stdio.h>

#include <cmath>

#include "mmloam_hip.h"

#define MML_POSE_INGEST_MAX 65535  // frames per call: the decode kernel's second grid dimension

// The decision for one frame.  np: the frame's six counts (union_cloud.msg order), row: its fetch row or nullptr (IMU_Mode == 0),
// first: this frame meets first_velo_frame == true.
inline mml_pose_ingest_row pose_ingest_decide(const int* np, const mml_imu_interval* row, bool first, const mml_pose_ingest_opts& o) {
    mml_pose_ingest_row r = {MML_INGEST_VELO_ONLY, MML_INGEST_WHY_MERGED, 0, 0, 0, 0};
    // :719-730  fetchImuMsgs returns !vimuMsg.empty(); after the retries the message is popped and the loop continues
    if (row && row->n == 0) {
        r.decision = MML_INGEST_DROPPED;
        r.reason = MML_INGEST_WHY_FETCH + row->status;
        return r;
    }
    const int n_velo = np[2], n_livox = np[5], livox_corner_num = np[3];
    r.n_points = r.n_velo = n_velo;
    if (!row) {  // :713, :741  IMU_Mode == 0: vimuMsg stays empty
        r.reason = MML_INGEST_WHY_NO_IMU;
        return r;
    }
    if (first) {  // :741, :838-839  first_velo_frame
        r.reason = MML_INGEST_WHY_FIRST_FRAME;
        return r;
    }
    const double front = row->front_gyro_z, back = row->back_gyro_z;
    if (o.velo_only_mode) {  // :746, :767
        r.reason = MML_INGEST_WHY_VELO_ONLY_MODE;
    } else if (!(std::abs(front) < o.hori_rotate_th || std::abs(back) < o.hori_rotate_th)) {  // :747, :763
        r.reason = MML_INGEST_WHY_FAST_ROTATION;
    } else if (!(livox_corner_num > 100)) {  // :748, :760
        r.reason = MML_INGEST_WHY_FEW_CORNERS;
    } else {  // :756  *laserCloudFullVeloRes + *laserCloudFullHoriRes
        r.decision = MML_INGEST_MERGED;
        r.reason = MML_INGEST_WHY_MERGED;
        r.n_points = n_velo + n_livox;
    }
    // :771  independent of the merge
    r.fast_rotation = (std::abs(front) > o.velo_rotate_th || std::abs(back) > o.velo_rotate_th) ? 1 : 0;
    return r;
}

// The checks that need no context, then the decisions of all frames into plan[0 .. count) -- a buffer of the caller's choice, so
// that a caller with more checks to make can keep `out` untouched.  Returns MML_OK or MML_ERR_INVALID with the text in msg
// (at least 160 characters).
inline int pose_ingest_plan(int count, const int* n_points, const mml_imu_interval* rows, const mml_pose_ingest_opts* opts,
                            mml_pose_ingest_row* plan, char* msg, size_t msg_len) {
    if (count < 1 || count > MML_POSE_INGEST_MAX) {
        snprintf(msg, msg_len, "count %d outside 1 .. %d", count, MML_POSE_INGEST_MAX);
        return MML_ERR_INVALID;
    }
    if (!n_points || !opts || !plan) {
        snprintf(msg, msg_len, "NULL n_points, opts or out");
        return MML_ERR_INVALID;
    }
    if (opts->first_frame < -1 || opts->first_frame >= count) {
        snprintf(msg, msg_len, "first_frame %d outside -1 .. %d", opts->first_frame, count - 1);
        return MML_ERR_INVALID;
    }
    for (int i = 0; i < count; ++i) {
        for (int k = 0; k < 6; ++k)
            if (n_points[6 * i + k] < 0) {
                snprintf(msg, msg_len, "frame %d: cloud %d has a negative count (%d)", i, k, n_points[6 * i + k]);
                return MML_ERR_INVALID;
            }
        if ((long long)n_points[6 * i + 2] + n_points[6 * i + 5] > INT_MAX) {
            snprintf(msg, msg_len, "frame %d: the two combine clouds together exceed INT_MAX points", i);
            return MML_ERR_INVALID;
        }
        if (rows && rows[i].n < 0) {
            snprintf(msg, msg_len, "frame %d: its fetch row has a negative count (%d)", i, rows[i].n);
            return MML_ERR_INVALID;
        }
    }
    for (int i = 0; i < count; ++i) plan[i] = pose_ingest_decide(n_points + 6 * i, rows ? rows + i : nullptr, i == opts->first_frame, *opts);
    return MML_OK;
}

#endif
