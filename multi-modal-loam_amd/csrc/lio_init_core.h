// lio_init_core.h -- the LIO initialisation of one segment (TryMAPInitialization, unionPoseEstimation.cpp:425-625), written once
// for the host loop of mml_lio_initialize_batch and for the device (k_lio_initialize, lio_init_batch.hip): lio_lm_solve, the
// joint problem's evaluation and lio_init_segment, steps 1-7 of mml_lio_initialize (lio_init.hip) for at most LIO_MAX_FRAMES
// frames with the whole state in one fixed struct.  It also OWNS what that single call shares with it and includes this header
// for: the cost functions (lio_quat_plus, lio_quat_plus_jacobian, lio_quat_rotate_wxyz, lio_cost_initial_g, lio_init_imu_raw),
// the Ceres constants and kLioGnorm.  The Cholesky and the 9 x 9 sqrt-information blocks are imu_math.h's, for both.
// lio_init.hip keeps its own lm_solve and steps 1-7 (any n, vectors sized by n); its header says why.  The routine here departs
// from that call's arithmetic in two places, the two where it reaches libm:
//   * lio_quat_plus takes mml_sin / mml_cos (its template argument; imu_math.h);
//   * the pre-integrations are not made here at all: the caller hands them in, made by imu_preint_interval<false> (imu_preint.h),
//     and redoes them with the new biases when the segment comes back with status 0.
// The host build runs every loop from 0 to its end on one thread.  The device build is called by ONE wavefront with the whole
// solve state (LioWork: the dense Jacobian, the normal matrix, lm_solve's vectors, the factors' blocks) in LDS, through the lane
// macros of marg_dense.h: MARG_FOR spreads independent elements over the lanes, MARG_LANE gives a sequential piece to one lane,
// MARG_SYNC orders the wavefront's LDS traffic.  A sum that mml_lio_initialize takes sequentially is taken sequentially here,
// by the lane that owns the output element, over i or k ascending from +0.0; a scalar every lane needs (the cost, the model
// change, the step norms, the Cholesky pivot) is summed by every lane from the same LDS values in that same order, so the
// control flow is uniform without a broadcast.  With -ffp-contract=off and correctly rounded sqrt and / the two builds are
// bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "imu_math.h"
#include "marg_dense.h"

namespace {

constexpr int LIO_MAX_FRAMES = 8;                                 // MML_LIO_BATCH_MAX_FRAMES
constexpr int LIO_NX = 9 + 3 * LIO_MAX_FRAMES;                    // 33 unknowns: r_wg | b_a | b_g | v_0 .. v_7
constexpr int LIO_M = LIO_NX + 9 * (LIO_MAX_FRAMES - 1);          // 96 residuals
constexpr int LIO_SQI = 192;                                      // doubles of work space per sqrt-information block
static_assert(sqrt_info_ws(9) <= LIO_SQI, "imu_math.h's sqrt_info_block on a 9 x 9 block");
static_assert((LIO_MAX_FRAMES - 1) * LIO_SQI <= LIO_M * LIO_NX, "the sqrt-information work space lies in LioWork::J");

constexpr double kLioGnorm = 9.805;  // IMUIntegrator.h:84, Cost_Initial_G / Cost_Initialization_IMU's G_I (0, 0, -9.805)
// Ceres 2.1.0 defaults (solver.h): max_num_iterations 50, function / gradient / parameter tolerance 1e-6 / 1e-10 / 1e-8,
// min_relative_decrease 1e-3, initial / max trust region radius 1e4 / 1e16, min radius 1e-32, LM diagonal clamp
// [1e-6, 1e32], 5 consecutive invalid steps end the solve (trust_region_minimizer.cc HandleInvalidStep).
constexpr int kLioMaxIter = 50;
constexpr double kLioFuncTol = 1e-6, kLioGradTol = 1e-10, kLioParamTol = 1e-8, kLioMinRelDecrease = 1e-3;
constexpr double kLioRadius0 = 1e4, kLioMaxRadius = 1e16, kLioMinRadius = 1e-32, kLioMinDiag = 1e-6, kLioMaxDiag = 1e32;

struct LioWork {
    double J[LIO_M * LIO_NX];  // local Jacobian of the current problem; before the solves the sqrt-information work space
    double A[LIO_NX * LIO_NX];
    double x[LIO_NX], x0[LIO_NX], xc[LIO_NX], g[LIO_NX], scale[LIO_NX], diag[LIO_NX], step[LIO_NX];
    double r[LIO_M], rc[LIO_M], mr[LIO_M];
    double Ja[12], Pj[12];                    // gravity problem: ambient Jacobian 3 x 4, QuaternionParameterization 4 x 3
    double U[(LIO_MAX_FRAMES - 1) * 81];      // sqrt information of factor f (frames f, f + 1): 9 x 9 upper
    double Jr[(LIO_MAX_FRAMES - 1) * 135];    // its raw Jacobian 9 x 15
    double rr[(LIO_MAX_FRAMES - 1) * 9];      // its raw residual
    double pb[3 * LIO_MAX_FRAMES], rb[3 * LIO_MAX_FRAMES], prior_v[3 * LIO_MAX_FRAMES], prior_r[3], avg[3];
    int ok[LIO_MAX_FRAMES];
};

struct LioProblem {  // what the two evaluations read besides LioWork
    bool quat;       // true: Cost_Initial_G on the quaternion; false: the joint problem
    int n;
    const mml_imu_preint* pre;  // n entries, entry 0 unused
};

// ---- imu_math.h's cholesky and chol_solve for the wavefront ------------------------------------------------------------------
// Column j: every lane takes the pivot's sum itself (the decision is uniform), the rows below are independent.  Only the lower
// triangle is read, as in the host form.
MARG_HD bool lio_cholesky_wave(double* A, int n) {
    for (int j = 0; j < n; ++j) {
        double d = A[j * n + j];
        for (int k = 0; k < j; ++k) d -= A[j * n + k] * A[j * n + k];
        if (!(d > 0.0) || !isfinite(d)) return false;
        d = sqrt(d);
        MARG_SYNC();  // every lane has read the pivot
        MARG_LANE(0) A[j * n + j] = d;
        MARG_FOR(ii, n - j - 1) {
            const int i = j + 1 + ii;
            double s = A[i * n + j];
            for (int k = 0; k < j; ++k) s -= A[i * n + k] * A[j * n + k];
            A[i * n + j] = s / d;
        }
        MARG_SYNC();
    }
    return true;
}
// Forwards column by column: row i meets its terms k ascending, the order of the row-by-row loop.  Backwards the row-by-row
// loop subtracts k ASCENDING from i + 1, which a column sweep from the last one down would reverse: one lane runs it as it is.
MARG_HD void lio_chol_solve_wave(const double* L, int n, double* b) {
    for (int k = 0; k < n; ++k) {
        MARG_LANE(0) b[k] = b[k] / L[k * n + k];
        MARG_SYNC();
        MARG_FOR(ii, n - k - 1) {
            const int i = k + 1 + ii;
            b[i] -= L[i * n + k] * b[k];
        }
        MARG_SYNC();
    }
    MARG_LANE(0) {
        for (int i = n - 1; i >= 0; --i) {
            double s = b[i];
            for (int k = i + 1; k < n; ++k) s -= L[k * n + i] * b[k];
            b[i] = s / L[i * n + i];
        }
    }
    MARG_SYNC();
}

// ---- the two cost functions ------------------------------------------------------------------------------------------------
// QuaternionParameterization::Plus, x = (w, x, y, z): [cos|d|, sin|d| / |d| d] (x) x; |d| = 0 leaves x as it is.  kLibm (imu_math.h's
// trig_sin / trig_cos): true in mml_lio_initialize's lm_solve alone, false in lio_lm_solve
template <bool kLibm>
MML_HD void lio_quat_plus(const double* x, const double* d, double* o) {
    const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (!(nd > 0.0)) {
        for (int i = 0; i < 4; ++i) o[i] = x[i];
        return;
    }
    const double s = trig_sin<kLibm>(nd) / nd;
    const double z[4] = {trig_cos<kLibm>(nd), s * d[0], s * d[1], s * d[2]};
    o[0] = z[0] * x[0] - z[1] * x[1] - z[2] * x[2] - z[3] * x[3];
    o[1] = z[0] * x[1] + z[1] * x[0] + z[2] * x[3] - z[3] * x[2];
    o[2] = z[0] * x[2] - z[1] * x[3] + z[2] * x[0] + z[3] * x[1];
    o[3] = z[0] * x[3] + z[1] * x[2] - z[2] * x[1] + z[3] * x[0];
}
MML_HD void lio_quat_plus_jacobian(const double* x, double* P) {  // 4 x 3 row-major
    P[0] = -x[1], P[1] = -x[2], P[2] = -x[3];
    P[3] = x[0], P[4] = x[3], P[5] = -x[2];
    P[6] = -x[3], P[7] = x[0], P[8] = x[1];
    P[9] = x[2], P[10] = -x[1], P[11] = x[0];
}
// Eigen's q * v for q = (w, x, y, z), not normalised
MML_HD void lio_quat_rotate_wxyz(const double* q, const double* v, double* o) {
    const double u[3] = {q[1], q[2], q[3]};
    double uv[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    for (int k = 0; k < 3; ++k) uv[k] += uv[k];
    const double c[3] = {u[1] * uv[2] - u[2] * uv[1], u[2] * uv[0] - u[0] * uv[2], u[0] * uv[1] - u[1] * uv[0]};
    for (int k = 0; k < 3; ++k) o[k] = v[k] + q[0] * uv[k] + c[k];
}
// Cost_Initial_G (ceresfunc.h:626-652): residual (3) and ambient Jacobian (3 x 4, columns w x y z; J may be NULL)
MML_HD void lio_cost_initial_g(const double* q, const double* acc, double* r, double* J) {
    const double v[3] = {0.0, 0.0, -kLioGnorm};
    lio_quat_rotate_wxyz(q, v, r);
    for (int k = 0; k < 3; ++k) r[k] -= acc[k];
    if (!J) return;
    const double u[3] = {q[1], q[2], q[3]};
    double uv[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    for (int k = 0; k < 3; ++k) uv[k] += uv[k];
    const M3 Vx = hat(v), UVx = hat(uv), Ux = hat(u);
    const M3 D = m3_add(m3_add(m3_scale(Vx, -2.0 * q[0]), m3_scale(UVx, -1.0)), m3_scale(m3_mul(Ux, Vx), -2.0));
    for (int i = 0; i < 3; ++i) {
        J[i * 4] = uv[i];
        for (int c = 0; c < 3; ++c) J[i * 4 + 1 + c] = D.a[3 * i + c];
    }
}
// Cost_Initialization_IMU (ceresfunc.h:654-741) before the sqrt information: residual (9) and, when J != NULL, the Jacobian
// (9 x 15, columns [rwg | vi | vj | ba | bg])
MML_HD void lio_init_imu_raw(const mml_imu_preint* pre, const double* ri, const double* rj, const double* dp, const double* rwg,
                             const double* vi, const double* vj, const double* ba, const double* bg, double* r, double* J) {
    const double G_I[3] = {0.0, 0.0, -kLioGnorm};
    const double dt = pre->dtime, dt2 = dt * dt;
    const double dbg[3] = {bg[0] - pre->bg[0], bg[1] - pre->bg[1], bg[2] - pre->bg[2]};
    const double dba[3] = {ba[0] - pre->ba[0], ba[1] - pre->ba[1], ba[2] - pre->ba[2]};
    const M3 Ri = so3_exp(ri), Rj = so3_exp(rj), Rwg = so3_exp(rwg), RiT = m3_t(Ri);
    const double* PJ = pre->jacobian;
    const M3 Jpbg = get_block(PJ, 15, 0, 9), Jpba = get_block(PJ, 15, 0, 12), Jrbg = get_block(PJ, 15, 3, 9),
             Jvbg = get_block(PJ, 15, 6, 9), Jvba = get_block(PJ, 15, 6, 12);
    double gw[3], a[3], b[3], Ra[3], Rb[3], t1[3], t2[3];
    m3_vec(Rwg, G_I, gw);
    for (int k = 0; k < 3; ++k) {
        a[k] = dp[k] - vi[k] * dt - gw[k] * dt2 * 0.5;
        b[k] = vj[k] - vi[k] - gw[k] * dt;
    }
    m3_vec(RiT, a, Ra);
    m3_vec(RiT, b, Rb);
    m3_vec(Jpbg, dbg, t1);
    m3_vec(Jpba, dba, t2);
    for (int k = 0; k < 3; ++k) r[k] = Ra[k] - (pre->dp[k] + t1[k] + t2[k]);
    double jd[3], rl[3];
    m3_vec(Jrbg, dbg, jd);
    const M3 C = m3_mul(quat_to_m3(pre->dq), so3_exp(jd));
    const M3 E = m3_mul(m3_t(C), m3_mul(RiT, Rj));
    so3_log(E, rl);
    for (int k = 0; k < 3; ++k) r[3 + k] = rl[k];
    m3_vec(Jvbg, dbg, t1);
    m3_vec(Jvba, dba, t2);
    for (int k = 0; k < 3; ++k) r[6 + k] = Rb[k] - (pre->dv[k] + t1[k] + t2[k]);
    if (!J) return;
    for (int i = 0; i < 9 * 15; ++i) J[i] = 0.0;
    // d(Rwg G_I) / d rwg = -Rwg [G_I]x Jr(rwg)
    const M3 dG = m3_mul(RiT, m3_mul(Rwg, m3_mul(hat(G_I), so3_Jr(rwg))));
    set_block(J, 15, 0, 0, dG, 0.5 * dt2);
    set_block(J, 15, 0, 3, RiT, -dt);
    set_block(J, 15, 0, 9, Jpba, -1.0);
    set_block(J, 15, 0, 12, Jpbg, -1.0);
    set_block(J, 15, 3, 12, m3_mul(so3_Jr_inv(rl), m3_mul(m3_t(E), m3_mul(so3_Jr(jd), Jrbg))), -1.0);
    set_block(J, 15, 6, 0, dG, dt);
    set_block(J, 15, 6, 3, RiT, -1.0);
    set_block(J, 15, 6, 6, RiT);
    set_block(J, 15, 6, 9, Jvba, -1.0);
    set_block(J, 15, 6, 12, Jvbg, -1.0);
}

// The joint problem over z = [r_wg | b_a | b_g | v_0 .. v_{n-1}] (unionPoseEstimation.cpp:498-576): residuals r (m) and, when
// J != NULL, the Jacobian (m x nx row-major).  The n - 1 IMU factors are evaluated one per lane; their sqrt-information products
// (eResiduals.applyOnTheLeft: sum over k = a .. 8 ascending from 0.0) one element per lane.
MML_HD void lio_joint_eval(const LioProblem& p, const double* z, double* r, double* J, LioWork& w) {
    const int n = p.n, nx = 9 + 3 * n, m = nx + 9 * (n - 1);
    if (J) {
        MARG_FOR(e, m * nx) J[e] = 0.0;
        MARG_SYNC();
    }
    MARG_LANE(0) {  // Cost_Initialization_Prior_R: 2000 log(exp(r)^-1 exp(prior_r)); d/dr = -Jr^-1(e) E^T Jr(r)
        const M3 Er = m3_mul(m3_t(so3_exp(z)), so3_exp(w.prior_r));
        double rl[3];
        so3_log(Er, rl);
        if (J) set_block(J, nx, 0, 0, m3_mul(so3_Jr_inv(rl), m3_mul(m3_t(Er), so3_Jr(z))), -2000.0);
        for (int k = 0; k < 3; ++k) r[k] = rl[k] * 2000.0;
    }
    // Cost_Initialization_Prior_bv: b_a (1000), b_g (4000) towards 0, v_i (4000) towards prior_v[i]
    MARG_FOR(k, 3) {
        r[3 + k] = 1000.0 * z[3 + k];
        r[6 + k] = 4000.0 * z[6 + k];
        if (J) {
            J[(3 + k) * nx + 3 + k] = 1000.0;
            J[(6 + k) * nx + 6 + k] = 4000.0;
        }
    }
    MARG_FOR(i, 3 * n) {
        r[9 + i] = 4000.0 * (z[9 + i] - w.prior_v[i]);
        if (J) J[(9 + i) * nx + 9 + i] = 4000.0;
    }
    // Cost_Initialization_IMU between frames f and f + 1 on (r_wg, v_f, v_{f+1}, b_a, b_g)
    MARG_FOR(f, n - 1) {
        double dp[3];
        for (int k = 0; k < 3; ++k) dp[k] = w.pb[3 * (f + 1) + k] - w.pb[3 * f + k];
        lio_init_imu_raw(p.pre + f + 1, w.rb + 3 * f, w.rb + 3 * (f + 1), dp, z, z + 9 + 3 * f, z + 9 + 3 * (f + 1), z + 3, z + 6,
                         w.rr + 9 * f, J ? w.Jr + 135 * f : nullptr);
    }
    MARG_SYNC();
    MARG_FOR(e, 9 * (n - 1)) {
        const int f = e / 9, a = e - 9 * f;
        const double* U = w.U + 81 * f;
        double s = 0;
        for (int k = a; k < 9; ++k) s += U[a * 9 + k] * w.rr[9 * f + k];
        r[nx + 9 * f + a] = s;
    }
    if (J) {
        MARG_FOR(e, 135 * (n - 1)) {
            const int f = e / 135, q = e - 135 * f, a = q / 15, c = q - 15 * a, b = c / 3, kk = c - 3 * b;
            const double* U = w.U + 81 * f;
            double s = 0;
            for (int k = a; k < 9; ++k) s += U[a * 9 + k] * w.Jr[135 * f + k * 15 + c];
            const int col = b == 0 ? 0 : b == 1 ? 9 + 3 * f : b == 2 ? 9 + 3 * (f + 1) : b == 3 ? 3 : 6;  // [rwg | vi | vj | ba | bg] -> z
            J[(nx + 9 * f + a) * nx + col + kk] += s;
        }
    }
    MARG_SYNC();
}

// residuals and, when J != NULL, the ambient Jacobian of problem p at z; returns with the wavefront's LDS traffic ordered
MML_HD void lio_eval(const LioProblem& p, const double* z, double* r, double* J, LioWork& w) {
    if (p.quat) {
        MARG_LANE(0) lio_cost_initial_g(z, w.avg, r, J);
        MARG_SYNC();
    } else {
        lio_joint_eval(p, z, r, J, w);
    }
}

MML_HD double lio_cost_of(const double* res, int m) {
    double c = 0;
    for (int i = 0; i < m; ++i) c += res[i] * res[i];
    return 0.5 * c;
}

// residuals, local Jacobian J = Ja * PlusJacobian, gradient J^T r at w.x; the projected gradient's max norm |x - Plus(x, -g)|_inf
// in gmax; returns the cost
MML_HD double lio_evaluate(const LioProblem& p, int na, int nl, int m, LioWork& w, double& gmax) {
    lio_eval(p, w.x, w.r, p.quat ? w.Ja : w.J, w);
    if (p.quat) {
        MARG_LANE(0) lio_quat_plus_jacobian(w.x, w.Pj);
        MARG_SYNC();
        MARG_FOR(e, m * nl) {
            const int i = e / nl, c = e - nl * i;
            double a = 0;
            for (int k = 0; k < na; ++k) a += w.Ja[i * na + k] * w.Pj[k * 3 + c];
            w.J[e] = a;
        }
        MARG_SYNC();
    }
    MARG_FOR(c, nl) {
        double a = 0;
        for (int i = 0; i < m; ++i) a += w.J[i * nl + c] * w.r[i];
        w.g[c] = a;
    }
    MARG_SYNC();
    gmax = 0;
    if (p.quat) {
        const double mg[3] = {-w.g[0], -w.g[1], -w.g[2]};
        double xp[4];
        lio_quat_plus<false>(w.x, mg, xp);
        for (int i = 0; i < 4; ++i) gmax = fmax(gmax, fabs(w.x[i] - xp[i]));
    } else {
        for (int i = 0; i < na; ++i) {
            const double mg = -w.g[i];
            const double xp = w.x[i] + mg;
            gmax = fmax(gmax, fabs(w.x[i] - xp));
        }
    }
    return lio_cost_of(w.r, m);
}

// lm_solve of lio_init.hip: Ceres 2.1.0's TrustRegionMinimizer with the LevenbergMarquardtStrategy on the dense problem p of m
// residuals over w.x (na ambient / nl tangent coordinates).  On FAILURE w.x is handed back as it came in.
MML_HD void lio_lm_solve(const LioProblem& p, int na, int nl, int m, LioWork& w, mml_solve_summary& s) {
    s.iterations = 0, s.successful = 0, s.initial_cost = 0.0, s.final_cost = 0.0, s.termination = 0;
    MARG_FOR(i, na) w.x0[i] = w.x[i];
    MARG_SYNC();
    double gmax = 0;
    double cost = lio_evaluate(p, na, nl, m, w, gmax);
    s.initial_cost = cost;
    // Jacobi scaling, fixed at the first evaluation: 1 / (1 + |column|)
    MARG_FOR(c, nl) {
        double a = 0;
        for (int i = 0; i < m; ++i) a += w.J[i * nl + c] * w.J[i * nl + c];
        w.scale[c] = 1.0 / (1.0 + sqrt(a));
    }
    MARG_SYNC();
    double radius = kLioRadius0, decrease = 2.0;
    bool reuse = false;
    int invalid = 0;
    for (;;) {  // at most kLioMaxIter rounds: every round that does not leave counts one iteration
        if (s.iterations >= kLioMaxIter) break;
        if (gmax <= kLioGradTol) {
            s.termination = 1;
            break;
        }
        if (radius < kLioMinRadius) break;
        s.iterations++;
        if (!reuse) {
            MARG_FOR(c, nl) {
                double a = 0;
                for (int i = 0; i < m; ++i) {
                    const double v = w.J[i * nl + c] * w.scale[c];
                    a += v * v;
                }
                w.diag[c] = fmin(fmax(a, kLioMinDiag), kLioMaxDiag);
            }
            MARG_SYNC();
        }
        // the lower triangle of Js^T Js + diag / radius (the Cholesky reads no more) and Js^T r
        MARG_FOR(e, nl * nl) {
            const int a = e / nl, b = e - nl * a;
            if (b <= a) {
                double h = 0;
                for (int i = 0; i < m; ++i) h += w.J[i * nl + a] * w.J[i * nl + b];
                double v = h * w.scale[a] * w.scale[b];
                if (a == b) v += w.diag[a] / radius;
                w.A[e] = v;
            }
        }
        MARG_FOR(a, nl) w.step[a] = w.g[a] * w.scale[a];
        MARG_SYNC();
        reuse = true;
        bool valid = lio_cholesky_wave(w.A, nl);
        if (valid) {
            lio_chol_solve_wave(w.A, nl, w.step);
            MARG_FOR(c, nl) w.step[c] = -w.step[c];
            MARG_SYNC();
            for (int c = 0; c < nl; ++c)
                if (!isfinite(w.step[c])) valid = false;
        }
        double model_change = 0;
        if (valid) {  // model_cost_change = -(Js step) . (r + Js step / 2)
            MARG_FOR(i, m) {
                double a = 0;
                for (int c = 0; c < nl; ++c) a += w.J[i * nl + c] * w.scale[c] * w.step[c];
                w.mr[i] = a;
            }
            MARG_SYNC();
            for (int i = 0; i < m; ++i) model_change += w.mr[i] * (w.r[i] + w.mr[i] / 2.0);
            model_change = -model_change;
            valid = model_change > 0.0;
        }
        if (!valid) {
            if (++invalid >= 5) {
                MARG_SYNC();
                MARG_FOR(i, na) w.x[i] = w.x0[i];
                MARG_SYNC();
                s.termination = 4;
                break;
            }
            radius /= decrease;
            decrease *= 2.0;
            continue;
        }
        invalid = 0;
        if (p.quat) {
            const double delta[3] = {w.step[0] * w.scale[0], w.step[1] * w.scale[1], w.step[2] * w.scale[2]};
            double xn[4];
            lio_quat_plus<false>(w.x, delta, xn);
            MARG_LANE(0) {
                for (int i = 0; i < 4; ++i) w.xc[i] = xn[i];
            }
        } else {
            MARG_FOR(i, na) {
                const double delta = w.step[i] * w.scale[i];
                w.xc[i] = w.x[i] + delta;
            }
        }
        MARG_SYNC();
        lio_eval(p, w.xc, w.rc, nullptr, w);
        const double cand = lio_cost_of(w.rc, m);
        double xn = 0, sn = 0;  // ParameterToleranceReached: the step measured in the ambient space
        for (int i = 0; i < na; ++i) {
            xn += w.x[i] * w.x[i];
            sn += (w.x[i] - w.xc[i]) * (w.x[i] - w.xc[i]);
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
        if (rho > kLioMinRelDecrease) {
            MARG_SYNC();  // every lane has read x
            MARG_FOR(i, na) w.x[i] = w.xc[i];
            MARG_SYNC();
            cost = lio_evaluate(p, na, nl, m, w, gmax);
            s.successful++;
            const double t = 2.0 * rho - 1.0;
            radius = fmin(kLioMaxRadius, radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
            decrease = 2.0;
            reuse = false;
        } else {
            radius /= decrease;
            decrease *= 2.0;
        }
    }
    s.final_cost = cost;
}

MML_HD void lio_put_summary(mml_solve_summary* d, const mml_solve_summary& s) {  // field by field: the padding stays zero
    d->iterations = s.iterations;
    d->successful = s.successful;
    d->initial_cost = s.initial_cost;
    d->final_cost = s.final_cost;
    d->termination = s.termination;
}

// Steps 1-7 of mml_lio_initialize on one segment of n frames (2 .. LIO_MAX_FRAMES), without the pre-integrations: pre[i]
// (i >= 1) is the one frame i holds.  t, P, Q, V, bg, ba: the segment's rows, written in place as that function writes them;
// samples0: the cnt0 >= 1 messages of frame 0; exTlb: 4 x 4.  *out receives the result.  Returns the status: 0 (the caller
// redoes the pre-integrations with the new biases), 1, 2, or 3 = pre[out->fail_frame]'s covariance is not positive definite,
// found before anything but *out is written.
MML_HD int lio_init_segment(int n, const double* t, double* P, double* Q, double* V, double* bg, double* ba, const double* samples0,
                            int cnt0, const double* exTlb, const mml_imu_preint* pre, mml_lio_init_result* out, LioWork& w) {
    MARG_LANE(0) {
        memset(out, 0, sizeof(*out));
        out->fail_frame = -1;
    }
    MARG_FOR(f, n - 1) w.ok[f] = sqrt_info_block(pre[f + 1].covariance, 15, 9, w.U + 81 * f, w.J + LIO_SQI * f) ? 1 : 0;
    MARG_SYNC();
    for (int f = 0; f + 1 < n; ++f)
        if (!w.ok[f]) {
            MARG_LANE(0) {
                out->status = 3;
                out->fail_frame = f + 1;
            }
            return 3;
        }
    const M3 exRlb = M3{{exTlb[0], exTlb[1], exTlb[2], exTlb[4], exTlb[5], exTlb[6], exTlb[8], exTlb[9], exTlb[10]}};  // :1456-1459
    const double exPlb[3] = {exTlb[3], exTlb[7], exTlb[11]};

    // 1. average_acc = -GetAverageAcc() of the first frame (the first 31 messages), rescaled to 9.805 (:428-432)
    double acc[3] = {0, 0, 0};
    int cnt = 0;
    for (int s = 0; s < cnt0; ++s) {
        const double* m = samples0 + 7 * (size_t)s;
        for (int k = 0; k < 3; ++k) acc[k] += m[3 + k] * kLioGnorm;
        cnt++;
        if (cnt > 30) break;
    }
    for (int k = 0; k < 3; ++k) acc[k] = -(acc[k] / cnt);
    const double an = sqrt(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2]);
    MARG_LANE(0) {
        for (int k = 0; k < 3; ++k) w.avg[k] = out->average_acc[k] = acc[k] * kLioGnorm / an;
        w.x[0] = 1.0;
        w.x[1] = w.x[2] = w.x[3] = 0.0;
    }
    MARG_SYNC();

    // 2. the gravity direction: Cost_Initial_G on para_quat = (1, 0, 0, 0), QuaternionParameterization (:436-455)
    LioProblem prob = {true, n, pre};
    mml_solve_summary sum;
    lio_lm_solve(prob, 4, 3, 3, w, sum);
    const double qwg[4] = {w.x[1], w.x[2], w.x[3], w.x[0]};  // (x, y, z, w)
    MARG_LANE(0) {
        lio_put_summary(&out->gravity_solve, sum);
        for (int k = 0; k < 4; ++k) out->q_wg[k] = qwg[k];
    }

    // 3. priors: prior_r = SO3(q_wg.toRotationMatrix()).log(), prior_v from the lidar positions moved to the body (:462-496)
    double prior_r[3];
    so3_log(quat_to_m3(qwg), prior_r);
    MARG_SYNC();  // every lane has read the gravity solve's x
    MARG_LANE(0) {
        for (int k = 0; k < 3; ++k) w.prior_r[k] = prior_r[k];
    }
    MARG_FOR(i, n) {
        const M3 R = quat_to_m3(Q + 4 * i);
        double Rp[3], rl[3];
        m3_vec(R, exPlb, Rp);
        for (int k = 0; k < 3; ++k) w.pb[3 * i + k] = P[3 * i + k] + Rp[k];
        so3_log(m3_mul(R, exRlb), rl);
        for (int k = 0; k < 3; ++k) w.rb[3 * i + k] = rl[k];
    }
    MARG_SYNC();
    MARG_FOR(e, 3 * n) {  // prior_v[0] = prior_v[1]
        const int i = e < 3 ? 1 : e / 3, k = e - 3 * (e / 3);
        w.prior_v[e] = (w.pb[3 * i + k] - w.pb[3 * (i - 1) + k]) / (t[i] - t[i - 1]);
    }
    MARG_SYNC();

    // 4. the joint problem over x = [r_wg | b_a | b_g | v_0 .. v_{n-1}] (:498-576)
    const int nx = 9 + 3 * n, m = nx + 9 * (n - 1);
    MARG_FOR(i, nx) w.x[i] = i < 9 ? 0.0 : w.prior_v[i - 9];
    MARG_SYNC();
    prob.quat = false;
    lio_lm_solve(prob, nx, nx, m, w, sum);

    // 5. GravityVector = exp(r_wg) (0, 0, -9.805) (:578-579)
    const double* x = w.x;
    const double G_I[3] = {0.0, 0.0, -kLioGnorm};
    const double rwg[3] = {x[0], x[1], x[2]};
    double grav[3];
    m3_vec(so3_exp(rwg), G_I, grav);
    MARG_LANE(0) {
        lio_put_summary(&out->joint_solve, sum);
        for (int k = 0; k < 3; ++k) {
            out->r_wg[k] = x[k];
            out->gravity[k] = grav[k];
            out->ba[k] = x[3 + k];
            out->bg[k] = x[6 + k];
        }
    }

    // 6. the checks, with the reference's partial writes (:581-600)
    const double nba = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]), nbg = sqrt(x[6] * x[6] + x[7] * x[7] + x[8] * x[8]);
    if (nba > 0.5 || nbg > 0.5) {
        MARG_LANE(0) out->status = 1;
        return 1;
    }
    for (int i = 0; i < n; ++i) {
        MARG_LANE(0) {
            for (int k = 0; k < 3; ++k) {
                ba[3 * i + k] = x[3 + k];
                bg[3 * i + k] = x[6 + k];
            }
        }
        const double* v = x + 9 + 3 * i;
        const double d0 = v[0] - w.prior_v[3 * i], d1 = v[1] - w.prior_v[3 * i + 1], d2 = v[2] - w.prior_v[3 * i + 2];
        if (sqrt(d0 * d0 + d1 * d1 + d2 * d2) > 2.0) {
            MARG_LANE(0) {
                out->status = 2;
                out->fail_frame = i;
            }
            return 2;
        }
        MARG_LANE(0) {
            for (int k = 0; k < 3; ++k) V[3 * i + k] = v[k];
        }
    }

    // 7. success: the list trimmed to SLIDEWINDOWSIZE = 5 (the caller drops frames before keep_from), the back frame alone moved
    //    from lidar to body (:612-619); the pre-integrations with the new biases (:602-609) are the caller's
    MARG_LANE(0) {
        out->keep_from = n > 5 ? n - 5 : 0;
        double* Pb = P + 3 * (n - 1);
        double* Qb = Q + 4 * (n - 1);
        const M3 R = quat_to_m3(Qb);
        double Rp[3], q[4];
        m3_vec(R, exPlb, Rp);
        for (int k = 0; k < 3; ++k) Pb[k] += Rp[k];
        m3_to_quat(m3_mul(R, exRlb), q);  // Quaterniond = Quaterniond * Matrix3d (a matrix, converted back)
        for (int k = 0; k < 4; ++k) Qb[k] = q[k];
    }
    return 0;
}

}  // namespace
