// imu_fetch.h -- the pose node's fetchImuMsgs (unionPoseEstimation.cpp:307-395) for one interval, GyroIntegration
// (IMUIntegrator.cpp:90-106) on the rows it cuts and the frame prediction of process() (:779-780, :805-828), shared by the host
// (mml_imu_fetch_host, mml_imu_predict_batch without a context) and the device (k_imu_plan, k_imu_write, k_imu_gyro,
// k_imu_predict, imu_stream.hip): the pattern of imu_preint.h and union_plan.h.  Plain double arithmetic in a fixed order,
// compiled with -ffp-contract=off on both sides, so the two builds give the same bytes.
//
// The queue is an array of messages, 7 doubles each (header.stamp.toSec(), angular_velocity xyz, linear_acceleration xyz),
// indexed ABSOLUTELY: i counts every message ever pushed, `front` is the first live one, `tail` one past the last; the array
// is indexed by i - origin.  The stamps T[front..tail) must not decrease (equal stamps are allowed).
//
// One interval (start, end], the checks in the reference's order:
//   :309, :327  no live message                              EMPTY        (1)
//   :325        end < start                                  REVERSED     (4)
//   :332        T[tail-1] < end                              NOT_REACHED  (2)
//   :338        T[front] >= end                              TOO_OLD      (3)
// Otherwise the walk of :344-379 (imu_idx from 0) skips every message with T <= start (:355), takes every message with
// start < T <= end (:348-351) and stops at the first T == end (:353) or at the first T > end, where it appends one message
// synthesised at `end` (:359-375).  On ordered stamps that is two searches:
//   lo = first i with T[i] >  start
//   hi = first i with T[i] >= end      (exists: T[tail-1] >= end)
//   T[hi] == end:  rows lo .. hi as they stand, interpolated = 0                                  (:348-353)
//   otherwise:     rows lo .. hi-1 and one row at `end` between messages hi-1 and hi               (:359-375):
//                  dt_1 = end - T[hi-1], dt_2 = T[hi] - end, w1 = dt_2 / (dt_1 + dt_2), w2 = dt_1 / (dt_1 + dt_2),
//                  each of the six values w1 * a + w2 * b
//   no message inside when the walk stops (lo >= hi with T[hi] > end; lo > hi with T[hi] == end, which needs end == start):
//                  the reference reads vimuMsg.back() of an empty vector, or -- end == start == T[tail-1] -- walks past the
//                  vector's end.  Defined here as NO_SAMPLE (5), no rows.  end == start always lands here.
// The synthesised message's stamp is `end` itself; the reference stores it through ros::Time::fromSec, which rounds to whole
// nanoseconds -- the identity for a stamp that came from a ROS header at epoch scale (doubles near 1.6e9 s are 238 ns apart),
// not for small synthetic times.  That is the one deliberate difference.
//
// Rows come out in the shape mml_imu_preintegrate takes: gyro xyz, accel xyz (message units), dt, where dt is the subtraction
// PreIntegration / GyroIntegration perform with lastTime = start (IMUIntegrator.cpp:122, :97): row 0 T - start, row k
// T_k - T_(k-1), the synthesised row end - T[hi-1].
#ifndef MML_IMU_FETCH_H
#define MML_IMU_FETCH_H

#include "imu_math.h"

enum { MML_IMU_FETCH_OK = 0, MML_IMU_FETCH_EMPTY = 1, MML_IMU_FETCH_NOT_REACHED = 2, MML_IMU_FETCH_TOO_OLD = 3, MML_IMU_FETCH_REVERSED = 4,
       MML_IMU_FETCH_NO_SAMPLE = 5 };

namespace {

MML_HD double imu_fetch_stamp(const double* msgs, long origin, long i) { return msgs[7 * (size_t)(i - origin)]; }

// First i in [lo, hi) with T[i] > t (kAfter) or T[i] >= t, else hi.
template <bool kAfter>
MML_HD long imu_fetch_bound(const double* msgs, long origin, long lo, long hi, double t) {
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        const double T = imu_fetch_stamp(msgs, origin, mid);
        if (kAfter ? T <= t : T < t)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Row k (0 <= k < n) of an OK interval whose first message is lo: out = gyro xyz, accel xyz, dt.
MML_HD void imu_fetch_row(const double* msgs, long origin, long lo, int n, int interpolated, double start, double end, int k, double* out) {
    const double* m = msgs + 7 * (size_t)(lo + k - origin);
    if (interpolated && k == n - 1) {  // (n >= 2: message hi - 1 is row n - 2)
        const double* a = m - 7;
        const double dt_1 = end - a[0], dt_2 = m[0] - end;
        const double w1 = dt_2 / (dt_1 + dt_2), w2 = dt_1 / (dt_1 + dt_2);
        for (int c = 0; c < 6; ++c) out[c] = w1 * a[1 + c] + w2 * m[1 + c];
        out[6] = end - a[0];
        return;
    }
    for (int c = 0; c < 6; ++c) out[c] = m[1 + c];
    out[6] = m[0] - (k == 0 ? start : m[-7]);
}

// The whole row of one interval: status, count, first message, and the gyro z of the first and last row it emits.
MML_HD void imu_fetch_plan(const double* msgs, long origin, long front, long tail, double start, double end, mml_imu_interval* r) {
    r->status = MML_IMU_FETCH_OK;
    r->n = 0;
    r->first = front;
    r->interpolated = 0;
    r->_pad = 0;
    r->front_gyro_z = r->back_gyro_z = 0.0;
    if (front >= tail) {
        r->status = MML_IMU_FETCH_EMPTY;
        return;
    }
    if (end < start) {
        r->status = MML_IMU_FETCH_REVERSED;
        return;
    }
    if (imu_fetch_stamp(msgs, origin, tail - 1) < end) {
        r->status = MML_IMU_FETCH_NOT_REACHED;
        return;
    }
    if (imu_fetch_stamp(msgs, origin, front) >= end) {
        r->status = MML_IMU_FETCH_TOO_OLD;
        return;
    }
    const long lo = imu_fetch_bound<true>(msgs, origin, front, tail, start);
    const long hi = imu_fetch_bound<false>(msgs, origin, front, tail, end);  // < tail on ordered stamps
    if (hi >= tail) {  // (unordered stamps only, which the callers refuse: nothing is read past the queue's end)
        r->status = MML_IMU_FETCH_NO_SAMPLE;
        return;
    }
    const int exact = imu_fetch_stamp(msgs, origin, hi) == end;
    const long n = hi - lo + 1;  // rows lo .. hi, or lo .. hi - 1 and the synthesised one
    if (n < 1 || (!exact && n < 2)) {
        r->status = MML_IMU_FETCH_NO_SAMPLE;
        return;
    }
    r->n = (int)n;  // (the caller bounds tail - front by 2^24)
    r->first = lo;
    r->interpolated = exact ? 0 : 1;
    double row[7];
    imu_fetch_row(msgs, origin, lo, r->n, r->interpolated, start, end, 0, row);
    r->front_gyro_z = row[2];
    imu_fetch_row(msgs, origin, lo, r->n, r->interpolated, start, end, r->n - 1, row);
    r->back_gyro_z = row[2];
}

// IMUIntegrator::GyroIntegration (IMUIntegrator.cpp:90-106) from the identity over n packed rows (gyro xyz, accel xyz, dt):
// the chain of mml_imu_gyro_integrate, sin / cos from imu_math.h.  q: x, y, z, w.
MML_HD void imu_fetch_gyro(const double* rows, int n, double* q_out) {
    double q[4] = {0.0, 0.0, 0.0, 1.0};
    for (int s = 0; s < n; ++s) {
        const double* m = rows + 7 * (size_t)s;
        const double dt = m[6];
        const double w[3] = {m[0] * dt, m[1] * dt, m[2] * dt};
        double qr[4];
        m3_to_quat(m3_mul(quat_to_m3(q), so3_exp(w)), qr);  // Quaterniond(dq * dR)
        if (qr[3] < 0)
            for (int k = 0; k < 4; ++k) qr[k] = -qr[k];
        const double nq = sqrt((qr[0] * qr[0] + qr[1] * qr[1]) + (qr[2] * qr[2] + qr[3] * qr[3]));
        for (int k = 0; k < 4; ++k) q[k] = qr[k] / nq;
    }
    for (int k = 0; k < 4; ++k) q_out[k] = q[k];
}

// ---- the frame prediction --------------------------------------------------------------------------------------------
// Hamilton product a * b and the rotation of a vector by a unit quaternion (q v q^*, written as v + w t + u x t with
// t = 2 u x v), both x, y, z, w.  Eigen's own operation order is not pinned: the tests hold these to a rounding bound.
MML_HD void imu_quat_mul(const double* a, const double* b, double* o) {
    o[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    o[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
    o[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
    o[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
}
MML_HD void imu_quat_rot(const double* q, const double* v, double* o) {
    const double t[3] = {2.0 * (q[1] * v[2] - q[2] * v[1]), 2.0 * (q[2] * v[0] - q[0] * v[2]), 2.0 * (q[0] * v[1] - q[1] * v[0])};
    o[0] = (v[0] + q[3] * t[0]) + (q[1] * t[2] - q[2] * t[1]);
    o[1] = (v[1] + q[3] * t[1]) + (q[2] * t[0] - q[0] * t[2]);
    o[2] = (v[2] + q[3] * t[2]) + (q[0] * t[1] - q[1] * t[0]);
}

// exTlb (4 x 4 row-major): R_lb = its rotation; exRbl = R_lb^T, exPbl = -R_lb^T t_lb (the inverse, as the adapter forms them).
struct ImuExtrinsic {
    M3 Rlb, Rbl;
    double Pbl[3], qbl[4];
};
MML_HD ImuExtrinsic imu_extrinsic(const double* exTlb) {
    ImuExtrinsic e;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) e.Rlb.a[3 * r + c] = exTlb[4 * r + c];
    e.Rbl = m3_t(e.Rlb);
    const double t[3] = {exTlb[3], exTlb[7], exTlb[11]};
    double p[3];
    m3_vec(e.Rbl, t, p);
    for (int k = 0; k < 3; ++k) e.Pbl[k] = -p[k];
    m3_to_quat(e.Rbl, e.qbl);  // Eigen::Quaterniond(exRbl)
    return e;
}

// :805-828.  prev: P(3) Q(4) V(3) of the previous frame; dq, dp, dv: the pre-integration's.  state: the predicted P(3) Q(4) V(3);
// delta_Rl (9, row-major) and delta_tl (3): velo_delta_Rl / velo_delta_tl, what mml_step / mml_undistort take as dR / dt.
MML_HD void imu_predict_lio(const double* prev, const double* dq, const double* dp, const double* dv, const ImuExtrinsic& e, double* state,
                            double* delta_Rl, double* delta_tl) {
    const double *Pp = prev, *Qp = prev + 3, *Vp = prev + 7;
    double P[3], Q[4], V[3], r[3];
    imu_quat_mul(Qp, dq, Q);  // :810
    imu_quat_rot(Qp, dp, r);
    for (int k = 0; k < 3; ++k) P[k] = Pp[k] + r[k];  // :812
    imu_quat_rot(Qp, dv, r);
    for (int k = 0; k < 3; ++k) V[k] = Vp[k] + r[k];  // :814
    double Qwlpre[4], Pwlpre[3], Qwl[4], Pwl[3];
    imu_quat_mul(Qp, e.qbl, Qwlpre);  // :819
    imu_quat_rot(Qp, e.Pbl, r);
    for (int k = 0; k < 3; ++k) Pwlpre[k] = r[k] + Pp[k];  // :820
    imu_quat_mul(Q, e.qbl, Qwl);  // :822
    imu_quat_rot(Q, e.Pbl, r);
    for (int k = 0; k < 3; ++k) Pwl[k] = r[k] + P[k];  // :823
    const double conj[4] = {-Qwlpre[0], -Qwlpre[1], -Qwlpre[2], Qwlpre[3]};
    double dql[4];
    imu_quat_mul(conj, Qwl, dql);  // :825
    const M3 Rl = quat_to_m3(dql);
    const double d[3] = {Pwl[0] - Pwlpre[0], Pwl[1] - Pwlpre[1], Pwl[2] - Pwlpre[2]};
    imu_quat_rot(conj, d, r);  // :826
    for (int k = 0; k < 3; ++k) {
        state[k] = P[k];
        state[7 + k] = V[k];
        delta_tl[k] = r[k];
    }
    for (int k = 0; k < 4; ++k) state[3 + k] = Q[k];
    for (int k = 0; k < 9; ++k) delta_Rl[k] = Rl.a[k];
}

// :779-780, the bring-up branch: velo_delta_Rb = dq.toRotationMatrix(), velo_delta_Rl = R_lb Rb R_lb^T.  gyro_Rb, gyro_Rl: 9 each.
MML_HD void imu_predict_gyro(const double* dq, const ImuExtrinsic& e, double* gyro_Rb, double* gyro_Rl) {
    const M3 Rb = quat_to_m3(dq);
    const M3 Rl = m3_mul(m3_mul(e.Rlb, Rb), e.Rbl);
    for (int k = 0; k < 9; ++k) {
        gyro_Rb[k] = Rb.a[k];
        gyro_Rl[k] = Rl.a[k];
    }
}

}  // namespace

#endif
