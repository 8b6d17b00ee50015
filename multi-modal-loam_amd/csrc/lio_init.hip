// lio_init.hip -- the LIO initialisation that opens the full-window (IMU_Mode 2) mode.  Host code: two dense problems of
// 4 and 9 + 3 n unknowns, solved once per session (retried every third scan until they succeed); the 15 W dogleg of
// window_imu.hip already showed that ONE serial dense solve of this size gains nothing on one wavefront.  Many of them at
// once are another matter: mml_lio_initialize_batch (lio_init_batch.hip, the routine in lio_init_core.h) runs a segment per
// wavefront for a replay of many segments; this file stays the single call.  Compiled into the same library so that it sits
// behind the same C-ABI.  What it owns is lm_solve and steps 1-7 of mml_lio_initialize; the cost functions (Cost_Initial_G,
// Cost_Initialization_IMU, the quaternion Plus and its Jacobian), the Ceres constants and kLioGnorm are lio_init_core.h's, the
// Cholesky and the sqrt information imu_math.h's, the pre-integration imu_preint.h's (through mml_imu_preintegrate) -- one text
// each for this call and the batch.  The only difference left in that shared text is libm's sin / cos here (lio_quat_plus<true>,
// imu_preint_interval<true>) against mml_sin / mml_cos there.
// lm_solve and lio_lm_solve (and the two texts of steps 1-7 around them) stay two routines ON PURPOSE: this call takes any
// n >= 2 and sizes its vectors by n (the reference's WINDOWSIZE is a run-time value, above 8 before the list is trimmed), the
// core keeps its whole state in a fixed LDS struct for at most MML_LIO_BATCH_MAX_FRAMES frames.  One routine for both would need
// pointer views, which cost the device its LDS addressing, or a bound on n here, which changes behaviour.
//   * IMUIntegrator::GyroIntegration        mm-loam/src/lio/IMUIntegrator.cpp:90-106      -> mml_imu_gyro_integrate
//   * IMUIntegrator::GetAverageAcc          IMUIntegrator.cpp:168-181                     -> (inside mml_lio_initialize)
//   * Cost_Initialization_IMU               mm-loam/include/utils/ceresfunc.h:654-741     -> mml_imu_init_factor
//     Jacobians: the reference lets Ceres autodiff the functors; here they are analytic (checked against central
//     differences in tests/test_lio_init.py)
//   * TryMAPInitialization                  mm-loam/src/unionPoseEstimation.cpp:425-625   -> mml_lio_initialize
//     Cost_Initial_G (ceresfunc.h:626-652) on a QuaternionParameterization, then Cost_Initialization_Prior_R / _bv / _IMU
//     (:654-818) jointly over r_wg, b_a, b_g and the frame velocities.
// Both ceres::Solve calls use default Solver::Options apart from DENSE_QR (:569-575), i.e. Ceres 2.1.0's
// LEVENBERG_MARQUARDT trust region; lm_solve below restates it once for both problems (convention 12:
// (J^T J + D^2) is solved by Cholesky where Ceres factors [J; D] by QR -- the same minimiser, different rounding).
#include <math.h>
#include <string.h>

#include <vector>

#include "imu_math.h"
#include "lio_init_core.h"

namespace {

// Ceres 2.1.0 TrustRegionMinimizer with the LevenbergMarquardtStrategy on a dense problem of m residuals over one
// parameter vector of na ambient / nl tangent coordinates (quat: the QuaternionParameterization, else Euclidean).
// eval(x, r, Ja) fills the residuals and, when Ja != NULL, the ambient Jacobian (m x na row-major).  x in/out; on
// FAILURE x is handed back as it came in (Solver::Solve leaves the user's parameters alone).
template <class Eval>
mml_solve_summary lm_solve(Eval eval, bool quat, int na, int nl, int m, double* x) {
    mml_solve_summary s = {0, 0, 0.0, 0.0, 0};
    std::vector<double> x0(x, x + na), xc(na), r(m), rc(m), Ja((size_t)m * na), J((size_t)m * nl), g(nl), scale(nl), diag(nl),
        A((size_t)nl * nl), step(nl), delta(nl), mr(m);
    auto plus = [&](const double* xa, const double* d, double* o) {
        if (quat)
            lio_quat_plus<true>(xa, d, o);  // libm: this call's results were pinned with it
        else
            for (int i = 0; i < na; ++i) o[i] = xa[i] + d[i];
    };
    auto cost_of = [&](const std::vector<double>& res) {
        double c = 0;
        for (int i = 0; i < m; ++i) c += res[i] * res[i];
        return 0.5 * c;
    };
    // residuals, local Jacobian J = Ja * PlusJacobian, gradient J^T r, and the projected gradient's max norm
    // |x - Plus(x, -g)|_inf (trust_region_minimizer.cc EvaluateGradientAndJacobian)
    double gmax = 0;
    auto evaluate = [&]() {
        eval(x, r.data(), Ja.data());
        if (quat) {
            double Pj[12];
            lio_quat_plus_jacobian(x, Pj);
            for (int i = 0; i < m; ++i)
                for (int c = 0; c < nl; ++c) {
                    double a = 0;
                    for (int k = 0; k < na; ++k) a += Ja[(size_t)i * na + k] * Pj[k * 3 + c];
                    J[(size_t)i * nl + c] = a;
                }
        } else {
            J = Ja;
        }
        for (int c = 0; c < nl; ++c) {
            double a = 0;
            for (int i = 0; i < m; ++i) a += J[(size_t)i * nl + c] * r[i];
            g[c] = a;
        }
        std::vector<double> mg(nl), xp(na);
        for (int c = 0; c < nl; ++c) mg[c] = -g[c];
        plus(x, mg.data(), xp.data());
        gmax = 0;
        for (int i = 0; i < na; ++i) gmax = fmax(gmax, fabs(x[i] - xp[i]));
        return cost_of(r);
    };
    double cost = evaluate();
    s.initial_cost = cost;
    // Jacobi scaling, fixed at the first evaluation: 1 / (1 + |column|)
    for (int c = 0; c < nl; ++c) {
        double a = 0;
        for (int i = 0; i < m; ++i) a += J[(size_t)i * nl + c] * J[(size_t)i * nl + c];
        scale[c] = 1.0 / (1.0 + sqrt(a));
    }
    double radius = kLioRadius0, decrease = 2.0;
    bool reuse = false;
    int invalid = 0;
    for (;;) {
        // FinalizeIterationAndCheckIfMinimizerCanContinue: iterations, gradient, minimum radius, in this order
        if (s.iterations >= kLioMaxIter) break;
        if (gmax <= kLioGradTol) {
            s.termination = 1;
            break;
        }
        if (radius < kLioMinRadius) break;
        s.iterations++;
        // LevenbergMarquardtStrategy::ComputeStep on the scaled Jacobian Js = J diag(scale):
        // (Js^T Js + diag / radius) y = Js^T r, step = -y; the diagonal (clamped squared column norms) is kept while
        // steps are rejected
        if (!reuse)
            for (int c = 0; c < nl; ++c) {
                double a = 0;
                for (int i = 0; i < m; ++i) {
                    const double v = J[(size_t)i * nl + c] * scale[c];
                    a += v * v;
                }
                diag[c] = fmin(fmax(a, kLioMinDiag), kLioMaxDiag);
            }
        for (int a = 0; a < nl; ++a) {
            for (int b = 0; b < nl; ++b) {
                double h = 0;
                for (int i = 0; i < m; ++i) h += J[(size_t)i * nl + a] * J[(size_t)i * nl + b];
                A[(size_t)a * nl + b] = h * scale[a] * scale[b];
            }
            A[(size_t)a * nl + a] += diag[a] / radius;
            step[a] = g[a] * scale[a];
        }
        reuse = true;
        bool valid = cholesky(A.data(), nl);
        if (valid) {
            chol_solve(A.data(), nl, step.data());
            for (int c = 0; c < nl; ++c) {
                step[c] = -step[c];
                if (!isfinite(step[c])) valid = false;
            }
        }
        double model_change = 0;
        if (valid) {  // model_cost_change = -(Js step) . (r + Js step / 2)
            for (int i = 0; i < m; ++i) {
                double a = 0;
                for (int c = 0; c < nl; ++c) a += J[(size_t)i * nl + c] * scale[c] * step[c];
                mr[i] = a;
            }
            for (int i = 0; i < m; ++i) model_change += mr[i] * (r[i] + mr[i] / 2.0);
            model_change = -model_change;
            valid = model_change > 0.0;
        }
        if (!valid) {  // HandleInvalidStep -> StepIsInvalid = StepRejected(0)
            if (++invalid >= 5) {
                for (int i = 0; i < na; ++i) x[i] = x0[i];
                s.termination = 4;
                break;
            }
            radius /= decrease;
            decrease *= 2.0;
            continue;
        }
        invalid = 0;
        for (int c = 0; c < nl; ++c) delta[c] = step[c] * scale[c];
        plus(x, delta.data(), xc.data());
        eval(xc.data(), rc.data(), nullptr);
        const double cand = cost_of(rc);
        // ParameterToleranceReached: the step measured in the ambient space
        double xn = 0, sn = 0;
        for (int i = 0; i < na; ++i) {
            xn += x[i] * x[i];
            sn += (x[i] - xc[i]) * (x[i] - xc[i]);
        }
        if (sqrt(sn) <= kLioParamTol * (sqrt(xn) + kLioParamTol)) {
            s.termination = 2;
            break;
        }
        if (fabs(cost - cand) <= kLioFuncTol * cost) {  // FunctionToleranceReached
            s.termination = 3;
            break;
        }
        const double rho = (cost - cand) / model_change;
        if (rho > kLioMinRelDecrease) {  // HandleSuccessfulStep + LevenbergMarquardtStrategy::StepAccepted
            for (int i = 0; i < na; ++i) x[i] = xc[i];
            cost = evaluate();
            s.successful++;
            const double t = 2.0 * rho - 1.0;
            radius = fmin(kLioMaxRadius, radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
            decrease = 2.0;
            reuse = false;
        } else {  // StepRejected
            radius /= decrease;
            decrease *= 2.0;
        }
    }
    s.final_cost = cost;
    return s;
}

void apply_upper(const double* U, int n, int cols, const double* in, double* out) {  // out = U in (U: n x n upper)
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < cols; ++c) {
            double s = 0;
            for (int k = i; k < n; ++k) s += U[i * n + k] * in[k * cols + c];
            out[i * cols + c] = s;
        }
}

}  // namespace

extern "C" {

int mml_imu_gyro_integrate(const double* samples, int n, double* dq) {
    if (!dq || n < 0 || (n > 0 && !samples)) return MML_ERR_INVALID;
    for (int s = 0; s < n; ++s)  // ROS_ASSERT(dt >= 0) (:97), checked before anything is written
        if (!(samples[7 * s + 6] >= 0.0)) return MML_ERR_INVALID;
    double q[4] = {dq[0], dq[1], dq[2], dq[3]};
    for (int s = 0; s < n; ++s) {
        const double* m = samples + 7 * s;
        const double dt = m[6];
        const double w[3] = {m[0] * dt, m[1] * dt, m[2] * dt};
        double qr[4];
        m3_to_quat(m3_mul(quat_to_m3(q), so3_exp(w)), qr);  // Quaterniond(dq * dR): toRotationMatrix() * dR -> quaternion
        if (qr[3] < 0)
            for (int k = 0; k < 4; ++k) qr[k] = -qr[k];
        const double nq = sqrt((qr[0] * qr[0] + qr[1] * qr[1]) + (qr[2] * qr[2] + qr[3] * qr[3]));
        for (int k = 0; k < 4; ++k) q[k] = qr[k] / nq;
    }
    for (int k = 0; k < 4; ++k) dq[k] = q[k];
    return MML_OK;
}

int mml_imu_init_factor(const mml_imu_preint* pre, const double* ri, const double* rj, const double* dp, const double* rwg,
                        const double* vi, const double* vj, const double* ba, const double* bg, double* residual,
                        double* jacobian) {
    if (!pre || !ri || !rj || !dp || !rwg || !vi || !vj || !ba || !bg || !residual) return MML_ERR_INVALID;
    double U[81], ws[sqrt_info_ws(9)];
    if (!sqrt_info_block(pre->covariance, 15, 9, U, ws)) return MML_ERR_STATE;
    double r[9], J[9 * 15];
    lio_init_imu_raw(pre, ri, rj, dp, rwg, vi, vj, ba, bg, r, jacobian ? J : nullptr);
    apply_upper(U, 9, 1, r, residual);  // eResiduals.applyOnTheLeft(sqrt_information)
    if (jacobian) apply_upper(U, 9, 15, J, jacobian);
    return MML_OK;
}

int mml_lio_initialize(int n, const double* t, double* P, double* Q, double* V, double* bg, double* ba, const double* samples,
                       const int* offsets, const double* exTlb, const mml_imu_preint* pre_in, mml_imu_preint* pre_out,
                       mml_lio_init_result* out) {
    if (n < 2 || !t || !P || !Q || !V || !bg || !ba || !samples || !offsets || !exTlb || !out) return MML_ERR_INVALID;
    for (int i = 0; i < n; ++i)
        if (offsets[i] < 0 || offsets[i + 1] < offsets[i]) return MML_ERR_INVALID;
    if (offsets[1] == offsets[0]) return MML_ERR_INVALID;  // GetAverageAcc would divide by zero
    memset(out, 0, sizeof(*out));
    out->fail_frame = -1;
    const M3 exRlb = M3{{exTlb[0], exTlb[1], exTlb[2], exTlb[4], exTlb[5], exTlb[6], exTlb[8], exTlb[9], exTlb[10]}};  // :1456-1459
    const double exPlb[3] = {exTlb[3], exTlb[7], exTlb[11]};
    // the pre-integration of every frame i >= 1 against frame i - 1: the caller's, or PreIntegration(t[i-1], bg[i-1], ba[i-1])
    std::vector<mml_imu_preint> pre(n);
    for (int i = 1; i < n; ++i) {
        if (pre_in) {
            pre[i] = pre_in[i];
        } else {
            const int rc = mml_imu_preintegrate(samples + 7 * (size_t)offsets[i], offsets[i + 1] - offsets[i], bg + 3 * i - 3,
                                                ba + 3 * i - 3, &pre[i]);
            if (rc != MML_OK) return rc;
        }
    }
    std::vector<double> U((size_t)81 * n);
    double ws[sqrt_info_ws(9)];
    for (int i = 1; i < n; ++i)
        if (!sqrt_info_block(pre[i].covariance, 15, 9, &U[81 * (size_t)i], ws)) return MML_ERR_STATE;

    // 1. average_acc = -GetAverageAcc() of the first frame (the first 31 messages), rescaled to 9.805 (:428-432)
    double acc[3] = {0, 0, 0};
    int cnt = 0;
    for (int s = offsets[0]; s < offsets[1]; ++s) {
        const double* m = samples + 7 * (size_t)s;
        for (int k = 0; k < 3; ++k) acc[k] += m[3 + k] * kLioGnorm;
        cnt++;
        if (cnt > 30) break;
    }
    for (int k = 0; k < 3; ++k) acc[k] = -(acc[k] / cnt);
    const double an = sqrt(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2]);
    for (int k = 0; k < 3; ++k) out->average_acc[k] = acc[k] * kLioGnorm / an;

    // 2. the gravity direction: Cost_Initial_G on para_quat = (1, 0, 0, 0), QuaternionParameterization (:436-455)
    double quat[4] = {1.0, 0.0, 0.0, 0.0};
    const double* avg = out->average_acc;
    out->gravity_solve = lm_solve([&](const double* q, double* r, double* J) { lio_cost_initial_g(q, avg, r, J); }, true, 4, 3, 3, quat);
    const double qwg[4] = {quat[1], quat[2], quat[3], quat[0]};  // (x, y, z, w)
    for (int k = 0; k < 4; ++k) out->q_wg[k] = qwg[k];

    // 3. priors: prior_r = SO3(q_wg.toRotationMatrix()).log(), prior_v from the lidar positions moved to the body (:462-496)
    double prior_r[3];
    so3_log(quat_to_m3(qwg), prior_r);
    std::vector<double> pb(3 * (size_t)n), rb(3 * (size_t)n), prior_v(3 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        const M3 R = quat_to_m3(Q + 4 * i);
        double Rp[3];
        m3_vec(R, exPlb, Rp);
        for (int k = 0; k < 3; ++k) pb[3 * i + k] = P[3 * i + k] + Rp[k];
        so3_log(m3_mul(R, exRlb), &rb[3 * i]);
    }
    for (int i = 1; i < n; ++i)
        for (int k = 0; k < 3; ++k) prior_v[3 * i + k] = (pb[3 * i + k] - pb[3 * (i - 1) + k]) / (t[i] - t[i - 1]);
    for (int k = 0; k < 3; ++k) prior_v[k] = prior_v[3 + k];

    // 4. the joint problem over x = [r_wg | b_a | b_g | v_0 .. v_{n-1}] (:498-576)
    const int nx = 9 + 3 * n, m = 9 + 3 * n + 9 * (n - 1);
    std::vector<double> x(nx, 0.0);
    for (int i = 0; i < 3 * n; ++i) x[9 + i] = prior_v[i];
    auto joint = [&](const double* z, double* r, double* J) {
        if (J) memset(J, 0, sizeof(double) * (size_t)m * nx);
        // Cost_Initialization_Prior_R: 2000 log(exp(r)^-1 exp(prior_r)); d/dr = -Jr^-1(e) E^T Jr(r)
        const M3 Er = m3_mul(m3_t(so3_exp(z)), so3_exp(prior_r));
        so3_log(Er, r);
        if (J) set_block(J, nx, 0, 0, m3_mul(so3_Jr_inv(r), m3_mul(m3_t(Er), so3_Jr(z))), -2000.0);
        for (int k = 0; k < 3; ++k) r[k] *= 2000.0;
        // Cost_Initialization_Prior_bv: b_a (1000), b_g (4000) towards 0, v_i (4000) towards prior_v[i]
        for (int k = 0; k < 3; ++k) {
            r[3 + k] = 1000.0 * z[3 + k];
            r[6 + k] = 4000.0 * z[6 + k];
            if (J) {
                J[(size_t)(3 + k) * nx + 3 + k] = 1000.0;
                J[(size_t)(6 + k) * nx + 6 + k] = 4000.0;
            }
        }
        for (int i = 0; i < 3 * n; ++i) {
            r[9 + i] = 4000.0 * (z[9 + i] - prior_v[i]);
            if (J) J[(size_t)(9 + i) * nx + 9 + i] = 4000.0;
        }
        // Cost_Initialization_IMU between frames i - 1 and i on (r_wg, v_{i-1}, v_i, b_a, b_g)
        for (int i = 1; i < n; ++i) {
            const int row = 9 + 3 * n + 9 * (i - 1);
            double dp[3], rr[9], Jr[9 * 15], Jw[9 * 15];
            for (int k = 0; k < 3; ++k) dp[k] = pb[3 * i + k] - pb[3 * (i - 1) + k];
            lio_init_imu_raw(&pre[i], &rb[3 * (i - 1)], &rb[3 * i], dp, z, z + 9 + 3 * (i - 1), z + 9 + 3 * i, z + 3, z + 6, rr,
                         J ? Jr : nullptr);
            apply_upper(&U[81 * (size_t)i], 9, 1, rr, r + row);
            if (!J) continue;
            apply_upper(&U[81 * (size_t)i], 9, 15, Jr, Jw);
            const int col[5] = {0, 9 + 3 * (i - 1), 9 + 3 * i, 3, 6};  // [rwg | vi | vj | ba | bg] -> x
            for (int a = 0; a < 9; ++a)
                for (int b = 0; b < 5; ++b)
                    for (int k = 0; k < 3; ++k) J[(size_t)(row + a) * nx + col[b] + k] += Jw[a * 15 + 3 * b + k];
        }
    };
    out->joint_solve = lm_solve(joint, false, nx, nx, m, x.data());

    // 5. GravityVector = exp(r_wg) (0, 0, -9.805) (:578-579)
    const double G_I[3] = {0.0, 0.0, -kLioGnorm};
    for (int k = 0; k < 3; ++k) out->r_wg[k] = x[k];
    m3_vec(so3_exp(x.data()), G_I, out->gravity);
    for (int k = 0; k < 3; ++k) {
        out->ba[k] = x[3 + k];
        out->bg[k] = x[6 + k];
    }
    if (pre_out)
        for (int i = 1; i < n; ++i) pre_out[i] = pre[i];

    // 6. the checks, with the reference's partial writes (:581-600)
    const double nba = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]), nbg = sqrt(x[6] * x[6] + x[7] * x[7] + x[8] * x[8]);
    if (nba > 0.5 || nbg > 0.5) {
        out->status = 1;
        return MML_OK;
    }
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) {
            ba[3 * i + k] = x[3 + k];
            bg[3 * i + k] = x[6 + k];
        }
        const double* v = &x[9 + 3 * i];
        const double d0 = v[0] - prior_v[3 * i], d1 = v[1] - prior_v[3 * i + 1], d2 = v[2] - prior_v[3 * i + 2];
        if (sqrt(d0 * d0 + d1 * d1 + d2 * d2) > 2.0) {
            out->status = 2;
            out->fail_frame = i;
            return MML_OK;
        }
        for (int k = 0; k < 3; ++k) V[3 * i + k] = v[k];
    }

    // 7. success: frame i + 1 pre-integrated again from frame i with frame i's new biases (:602-609), the list trimmed to
    //    SLIDEWINDOWSIZE = 5 (the caller drops frames before keep_from), the back frame alone moved from lidar to body (:612-619)
    for (int i = 0; i + 1 < n; ++i) {
        const int rc = mml_imu_preintegrate(samples + 7 * (size_t)offsets[i + 1], offsets[i + 2] - offsets[i + 1], bg + 3 * i,
                                            ba + 3 * i, &pre[i + 1]);
        if (rc != MML_OK) return rc;
        if (pre_out) pre_out[i + 1] = pre[i + 1];
    }
    out->keep_from = n > 5 ? n - 5 : 0;
    {
        double* Pb = P + 3 * (n - 1);
        double* Qb = Q + 4 * (n - 1);
        const M3 R = quat_to_m3(Qb);
        double Rp[3], q[4];
        m3_vec(R, exPlb, Rp);
        for (int k = 0; k < 3; ++k) Pb[k] += Rp[k];
        m3_to_quat(m3_mul(R, exRlb), q);  // Quaterniond = Quaterniond * Matrix3d (a matrix, converted back)
        for (int k = 0; k < 4; ++k) Qb[k] = q[k];
    }
    return MML_OK;
}

}  // extern "C"
