// imu_preint.h -- the pre-integration of one IMU interval (IMUIntegrator::PreIntegration, IMUIntegrator.cpp:108-166): n samples
// and the linearisation biases in, one mml_imu_preint out.  The ONE text of it: mml_imu_preintegrate (window_imu.hip), the host
// loops of mml_imu_preintegrate_batch and mml_lio_initialize_batch, and the device (k_imu_preintegrate, imu_preint.hip;
// k_lio_preint, lio_init_batch.hip) all run imu_preint_interval.  Its template argument chooses the right Jacobian's sin / cos
// (trig_sin / trig_cos, imu_math.h) -- the one place where a host build and a device build could part:
//   * kLibm = true, libm: mml_imu_preintegrate alone, whose results were pinned with it;
//   * kLibm = false, mml_sin / mml_cos: every batch caller, host and device.
// The right Jacobian feeds only the Jacobian and covariance chains, so the two forms give the same dp, dv, dq, dtime, bg, ba
// always, and the same bytes throughout wherever no step rotates by more than 1e-5 rad.
// A and B are used by their block structure: A is the identity plus seven 3 x 3 blocks, B five blocks, and a dot product adds
// the terms of the entries that are not structurally zero, ascending k, to an accumulator that starts at +0.0.  A dense
// 15 x 15 loop would add +-0.0 for every other k, which never changes such an accumulator (it cannot hold -0.0), so for finite
// samples the result has the bytes of the dense products (0 * inf is the exception: with a non-finite sample the output is
// unspecified).
// The host build runs every loop from 0 to its end on one thread.  The device build is called by ONE wavefront with the work
// space in LDS, the way marg_dense.h is (its macros): what depends on one sample only -- exp(gyr dt), the right Jacobian, the
// bias-corrected acceleration -- is computed for a chunk of samples at a time, a sample per lane (MARG_FOR); the chain over the
// samples then costs, per sample, the 3 x 3 work on dq / dp / dv, which every lane carries in registers and computes from the same
// values, and the three 15 x 15 products, one element per lane and pass, every sum in the host's order.  With
// -ffp-contract=off and correctly rounded sqrt and / on both sides the two builds are bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "imu_math.h"
#include "marg_dense.h"

namespace {

constexpr int PREINT_CHUNK = 32;  // samples per chunk: their sample-only terms are computed side by side
constexpr int PREINT_REC = 22;    // per sample: dR^T (9) | Jr (9) | acc (3) | dt

constexpr double kPreGnorm = 9.805;                                                    // IMUIntegrator.h:84
constexpr double kPreAccN = 0.08, kPreGyrN = 0.004, kPreAccW = 2.0e-4, kPreGyrW = 2.0e-5;  // IMUIntegrator.h:79-82

struct PreintWork {
    double jac[2][225];  // the Jacobian before / after a sample, alternating
    double cov[225];
    double T[225];  // A * covariance; between two chunks the raw samples of the next one (PREINT_CHUNK x 7)
    double rec[PREINT_CHUNK][PREINT_REC];
    double Rq[9], RqA[9];  // dq.matrix(), dq.matrix() * hat(acc) of the current sample
};
static_assert(PREINT_CHUNK * 7 <= 225, "a chunk of raw samples is staged in PreintWork::T");

// what one sample contributes on its own (:119-135): m = gyro xyz, accel xyz (message units), dt
template <bool kLibm>
MARG_HD void preint_sample_terms(const double* m, const double* bg, const double* ba, double* rec) {
    const double gyr[3] = {m[0] - bg[0], m[1] - bg[1], m[2] - bg[2]};
    const double dt = m[6];
    const double gdt[3] = {gyr[0] * dt, gyr[1] * dt, gyr[2] * dt};
    const M3 dRt = m3_t(so3_exp(gdt));
    M3 Jr = m3_identity();
    const double nrm = sqrt((gdt[0] * gdt[0] + gdt[1] * gdt[1]) + gdt[2] * gdt[2]);
    if (nrm > 0.00001) {  // :129-135
        const double k[3] = {gdt[0] / nrm, gdt[1] / nrm, gdt[2] / nrm};
        const M3 K = hat(k);
        // (1 - cos nrm) / nrm as 2 sin^2(nrm / 2) / nrm: the difference cancels (4e-7 relative at nrm = 1.01e-5)
        const double sh = trig_sin<kLibm>(0.5 * nrm);
        Jr = m3_add(m3_add(m3_identity(), m3_scale(K, -(2.0 * (sh * sh)) / nrm)), m3_scale(m3_mul(K, K), 1 - trig_sin<kLibm>(nrm) / nrm));
    }
    for (int i = 0; i < 9; ++i) {
        rec[i] = dRt.a[i];
        rec[9 + i] = Jr.a[i];
    }
    for (int i = 0; i < 3; ++i) rec[18 + i] = m[3 + i] * kPreGnorm - ba[i];
    rec[21] = dt;
}

// sum over k ascending of A[row][k] * X[k * stride], over the entries of that row of A which are not structurally zero:
//   rows 0-2   1 | -0.5 dt2 Rq hat(acc) (cols 3-5) | dt (col 6 + row) | -0.5 dt2 Rq (cols 12-14)
//   rows 3-5   dR^T (cols 3-5) | -dt Jr (cols 9-11)
//   rows 6-8   -dt Rq hat(acc) (cols 3-5) | 1 | -dt Rq (cols 12-14)
//   rows 9-14  1
// Every entry is formed as set_block forms it: scale * block element.
MARG_HD double preint_A_dot(const PreintWork& w, const double* rec, double dt, double dt2, int row, const double* X, int stride) {
    double acc = 0.0;
    if (row < 3) {
        const double s = -0.5 * dt2;
        acc += X[row * stride];
        for (int j = 0; j < 3; ++j) acc += (s * w.RqA[3 * row + j]) * X[(3 + j) * stride];
        acc += dt * X[(6 + row) * stride];
        for (int j = 0; j < 3; ++j) acc += (s * w.Rq[3 * row + j]) * X[(12 + j) * stride];
    } else if (row < 6) {
        const int q = row - 3;
        const double s = -dt;
        for (int j = 0; j < 3; ++j) acc += rec[3 * q + j] * X[(3 + j) * stride];
        for (int j = 0; j < 3; ++j) acc += (s * rec[9 + 3 * q + j]) * X[(9 + j) * stride];
    } else if (row < 9) {
        const int q = row - 6;
        const double s = -dt;
        for (int j = 0; j < 3; ++j) acc += (s * w.RqA[3 * q + j]) * X[(3 + j) * stride];
        acc += X[row * stride];
        for (int j = 0; j < 3; ++j) acc += (s * w.Rq[3 * q + j]) * X[(12 + j) * stride];
    } else {
        acc += X[row * stride];
    }
    return acc;
}

// (B noise B^T)[r][c] = sum over k ascending of (B[r][k] * noise[k]) * B[c][k].  Rows of B:
//   0-2  0.5 dt2 Rq (cols 3-5) | 3-5  dt Jr (cols 0-2) | 6-8  dt Rq (cols 3-5) | 9-14  dt (col row - 3)
// noise = diag(gyr_n^2 x 3, acc_n^2 x 3, gyr_w^2 x 3, acc_w^2 x 3) (:33-37)
MARG_HD double preint_BnB(const PreintWork& w, const double* rec, double dt, double dt2, int r, int c) {
    double bn = 0.0;
    if (r >= 9 || c >= 9) {
        if (r == c) bn += (dt * (r < 12 ? kPreGyrW * kPreGyrW : kPreAccW * kPreAccW)) * dt;
        return bn;
    }
    const bool rot_r = r >= 3 && r < 6, rot_c = c >= 3 && c < 6;
    if (rot_r != rot_c) return bn;
    if (rot_r) {
        for (int j = 0; j < 3; ++j) bn += ((dt * rec[9 + 3 * (r - 3) + j]) * (kPreGyrN * kPreGyrN)) * (dt * rec[9 + 3 * (c - 3) + j]);
    } else {
        const double sr = r < 3 ? 0.5 * dt2 : dt, sc = c < 3 ? 0.5 * dt2 : dt;
        const int qr = r < 3 ? r : r - 6, qc = c < 3 ? c : c - 6;
        for (int j = 0; j < 3; ++j) bn += ((sr * w.Rq[3 * qr + j]) * (kPreAccN * kPreAccN)) * (sc * w.Rq[3 * qc + j]);
    }
    return bn;
}

// samples: n x 7 (n >= 0); bg, ba: 3 each.  n = 0 gives Reset() (:49-58).
template <bool kLibm>
MARG_HD void imu_preint_interval(const double* samples, int n, const double* bg_, const double* ba_, mml_imu_preint* out, PreintWork& w) {
    const double bg[3] = {bg_[0], bg_[1], bg_[2]}, ba[3] = {ba_[0], ba_[1], ba_[2]};
    double dq[4] = {0.0, 0.0, 0.0, 1.0}, dp[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0}, dtime = 0.0;
    int cur = 0;
    MARG_FOR(e, 225) {
        w.jac[0][e] = (e / 15 == e % 15) ? 1.0 : 0.0;
        w.cov[e] = 0.0;
    }
    MARG_SYNC();
    for (int s0 = 0; s0 < n; s0 += PREINT_CHUNK) {
        const int cnt = n - s0 < PREINT_CHUNK ? n - s0 : PREINT_CHUNK;
        MARG_FOR(e, 7 * cnt) w.T[e] = samples[7 * (size_t)s0 + e];
        MARG_SYNC();
        MARG_FOR(i, cnt) preint_sample_terms<kLibm>(w.T + 7 * i, bg, ba, w.rec[i]);
        MARG_SYNC();
        for (int i = 0; i < cnt; ++i) {
            const double* rec = w.rec[i];
            const double acc[3] = {rec[18], rec[19], rec[20]};
            const double dt = rec[21], dt2 = dt * dt;
            const M3 Rq = quat_to_m3(dq);
            const M3 RqA = m3_mul(Rq, hat(acc));
            MARG_LANE(0) {
                for (int k = 0; k < 9; ++k) {
                    w.Rq[k] = Rq.a[k];
                    w.RqA[k] = RqA.a[k];
                }
            }
            MARG_SYNC();
            // jacobian = A * jacobian, T = A * covariance
            const double* J = w.jac[cur];
            double* Jn = w.jac[cur ^ 1];
            MARG_FOR(e, 225) {
                const int r = e / 15, c = e - 15 * r;
                Jn[e] = preint_A_dot(w, rec, dt, dt2, r, J + c, 15);
                w.T[e] = preint_A_dot(w, rec, dt, dt2, r, w.cov + c, 15);
            }
            cur ^= 1;
            MARG_SYNC();
            // covariance = T * A^T + B * noise * B^T
            MARG_FOR(e, 225) {
                const int r = e / 15, c = e - 15 * r;
                const double acc_ = preint_A_dot(w, rec, dt, dt2, c, w.T + 15 * r, 1);
                const double bn = preint_BnB(w, rec, dt, dt2, r, c);
                w.cov[e] = acc_ + bn;
            }
            // dp += dv*dt + 0.5*dq*acc*dt2 ; dv += dq*acc*dt   (:159-160)
            double Ra[3];
            m3_vec(Rq, acc, Ra);
            for (int k = 0; k < 3; ++k) dp[k] += dv[k] * dt + 0.5 * Ra[k] * dt2;
            for (int k = 0; k < 3; ++k) dv[k] += Ra[k] * dt;
            // dq = normalized(Quaterniond(dq.matrix() * dR)), w >= 0  (:161-165)
            const M3 dR = M3{{rec[0], rec[3], rec[6], rec[1], rec[4], rec[7], rec[2], rec[5], rec[8]}};
            double q[4];
            m3_to_quat(m3_mul(Rq, dR), q);
            if (q[3] < 0)
                for (int k = 0; k < 4; ++k) q[k] = -q[k];
            const double nq = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
            for (int k = 0; k < 4; ++k) dq[k] = q[k] / nq;
            dtime += dt;
            MARG_SYNC();  // the next sample replaces Rq / RqA, the next chunk T and rec
        }
    }
    MARG_FOR(e, 225) {
        out->jacobian[e] = w.jac[cur][e];
        out->covariance[e] = w.cov[e];
    }
    MARG_LANE(0) {
        for (int k = 0; k < 3; ++k) {
            out->dp[k] = dp[k];
            out->dv[k] = dv[k];
            out->bg[k] = bg[k];
            out->ba[k] = ba[k];
        }
        for (int k = 0; k < 4; ++k) out->dq[k] = dq[k];
        out->dtime = dtime;
    }
}

}  // namespace
