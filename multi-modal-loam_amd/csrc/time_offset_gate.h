// time_offset_gate.h -- which queued Velodyne frame LidarsParamEstimator::estimate_timeoffset runs on
// (unionLidarsAligner.cpp:1026-1051), as ONE host routine behind mml_time_offset_gate.  Host code only, no HIP: a program without
// kernels can include it.
//
// `abs` at :1034 is the unqualified call on a double (a difference of two ros::Time::toSec()).  The TU includes <tf/tf.h> (:9) ->
// tf/LinearMath/Scalar.h -> <math.h>, and libstdc++'s <math.h> (gcc >= 6; melodic: 7.5) adds `using std::abs;` to the global
// namespace; the TU has no using-directive of its own.  Overload resolution takes std::abs(double), not the C library's abs(int)
// (which would truncate every difference below one second to 0 and pop every frame).  DESIGN.md section 2, convention 15.
#ifndef MML_TIME_OFFSET_GATE_H
#define MML_TIME_OFFSET_GATE_H

#include <stdint.h>

#include <cmath>

#include "mmloam_hip.h"

// ros::Time::toSec() (rostime time.h) of the stamp ns: sec = ns / 1e9 and nsec = ns % 1e9 as ros::Time holds them
inline double tofs_gate_to_sec(uint64_t ns) { return (double)(ns / 1000000000ull) + 1e-9 * (double)(ns % 1000000000ull); }

inline int time_offset_gate(int n_velo, const uint64_t* velo_stamps, uint64_t hori_stamp, int n_hori_msgs, int* selected, int* status) {
    if (n_velo < 0 || n_hori_msgs < 0 || (n_velo > 0 && !velo_stamps) || !selected || !status) return MML_ERR_INVALID;
    *selected = -1;
    if (n_velo == 0) {  // :1026  back() of an empty vector
        *status = MML_TOFS_GATE_EMPTY;
        return MML_OK;
    }
    int k = n_velo - 1;                                // :1026  velo_vec.back()
    const double hori = tofs_gate_to_sec(hori_stamp);  // :1027, :1040  hori_vec is not popped: the same stamp every round
    double velo = tofs_gate_to_sec(velo_stamps[k]);
    while (velo > hori || std::abs(velo - hori) < 0.2) {  // :1034
        if (k == 0) {  // :1037-1039  the last frame is popped and back() reads an empty vector
            *status = MML_TOFS_GATE_EMPTY;
            return MML_OK;
        }
        --k;  // :1037-1038
        velo = tofs_gate_to_sec(velo_stamps[k]);  // :1039
    }
    if (n_hori_msgs < 8) {  // :1051  hori_vec[msg_size - 8] lies before the vector's start
        *status = MML_TOFS_GATE_TOO_FEW_MESSAGES;
        return MML_OK;
    }
    *selected = k;  // :1044
    *status = MML_TOFS_GATE_OK;
    return MML_OK;
}

#endif
