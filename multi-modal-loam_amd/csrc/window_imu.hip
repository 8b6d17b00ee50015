// window_imu.hip -- SURVEY.md section 8(f) rank 1: the IMU side of the joint window solve.  Host code (W <= 8 frames,
// 15 parameters each: O(W) tiny dense work next to the per-frame lidar normal equations that come from the device),
// compiled into the same library so that it sits behind the same C-ABI; the same trust-region loop resident on the
// device is fullwindow_dev.hip, the shared arithmetic imu_math.h (IMU residual and Jacobian, the sqrt-information
// products imu_whiten, the prior residual, the sequential Cholesky and sqrt_info_block) and lidar_eval.h's Hget for a
// record's upper triangle.  This file owns the trust-region loop, the factor's entry points and chol_solve_rcp.
//   * IMUIntegrator::PreIntegration            mm-loam/src/lio/IMUIntegrator.cpp:108-166  -> mml_imu_preintegrate
//     (the argument checks here; the arithmetic is imu_preint.h's imu_preint_interval, the batch calls' routine)
//   * Cost_NavState_PRV_Bias (15 residuals)    mm-loam/include/utils/ceresfunc.h:321-393   -> mml_imu_factor
//     Jacobians: the reference lets Ceres autodiff the functor; here they are analytic (checked against central
//     differences of the residual in tests/test_imu.py)
//   * MarginalizationInfo / MarginalizationFactor  ceresfunc.h:92-317, hookup Estimator.cpp:1448-1567
//                                                                                          -> mml_fullwindow_marginalize
//   * the full-window problem of Estimator::Estimate (Estimator.cpp:1226-1254,1425-1432): lidar blocks on para_PR[f],
//     IMU factors between consecutive frames on (para_PR, para_VBias), the marginalization prior on frame 0, solved
//     with the same trust-region dogleg iteration as mml_solve but on the dense 15 W system     -> mml_fullwindow_*
// Rotation blocks are rotation VECTORS in a plain Euclidean parameter block (Estimator.cpp:1228), R = Sophus exp.
#include <math.h>
#include <string.h>

#include <vector>

#include "fullwindow_internal.h"
#include "imu_math.h"
#include "imu_preint.h"
#include "lidar_eval.h"
#include "marg_dense.h"

namespace {

// imu_math.h's chol_solve with the reciprocals of the diagonal taken once and multiplied in: the form the device-resident solver
// (fullwindow_dev.hip) uses, where a division would sit on the dependency chain of every substitution step.  The terms of a
// row are subtracted in the order a column-by-column (right-looking) substitution meets them -- ascending k forwards,
// DESCENDING k backwards, "the columns become known from the last one down" -- which is the device's order: the two
// iterations then hold bit-identical steps.
void chol_solve_rcp(const double* L, int n, double* b) {
    std::vector<double> rd(n);
    for (int i = 0; i < n; ++i) rd[i] = 1.0 / L[i * n + i];
    for (int i = 0; i < n; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s -= L[i * n + k] * b[k];
        b[i] = s * rd[i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = b[i];
        for (int k = n - 1; k > i; --k) s -= L[k * n + i] * b[k];
        b[i] = s * rd[i];
    }
}
// sqrt information of one pre-integration: LLT(covariance^-1).matrixL().transpose() (Estimator.cpp:1240-1242)
bool imu_sqrt_info(const mml_imu_preint* pre, double* U /*15x15 upper*/) {
    double ws[sqrt_info_ws(15)];
    return sqrt_info_block(pre->covariance, 15, 15, U, ws);
}

}  // namespace

extern "C" {

// imu_preint.h's routine with libm in the right Jacobian.  Sample values are not checked; with a non-finite sample the output is
// unspecified.
int mml_imu_preintegrate(const double* samples, int n, const double* bg, const double* ba, mml_imu_preint* out) {
    if (!out || n < 0 || (n > 0 && !samples) || !bg || !ba) return MML_ERR_INVALID;
    PreintWork work;
    imu_preint_interval<true>(samples, n, bg, ba, out, work);
    return MML_OK;
}

static void imu_factor_with_U(const mml_imu_preint* pre, const double* U, const double* gravity, const double* pri, const double* vbi,
                              const double* prj, const double* vbj, double* residual, double* jacobian);

int mml_imu_factor(const mml_imu_preint* pre, const double* gravity, const double* pri, const double* vbi, const double* prj,
                   const double* vbj, double* residual, double* jacobian) {
    if (!pre || !gravity || !pri || !vbi || !prj || !vbj || !residual) return MML_ERR_INVALID;
    double U[225];
    if (!imu_sqrt_info(pre, U)) return MML_ERR_STATE;
    imu_factor_with_U(pre, U, gravity, pri, vbi, prj, vbj, residual, jacobian);
    return MML_OK;
}

// the factor for a sqrt information that is already known (the full-window solver factors each covariance once, when the
// pre-integration is handed over, instead of once per evaluation)
static void imu_factor_with_U(const mml_imu_preint* pre, const double* U, const double* gravity, const double* pri, const double* vbi,
                              const double* prj, const double* vbj, double* residual, double* jacobian) {
    double r[15], J[15 * 30];
    imu_raw(pre, gravity, pri, vbi, prj, vbj, r, jacobian ? J : nullptr);
    for (int o = jacobian ? 0 : 450; o < 465; ++o) (o < 450 ? jacobian[o] : residual[o - 450]) = imu_whiten(U, J, r, o);
}

}  // extern "C"

// ---- the full-window problem -------------------------------------------------------------------------------------------
namespace {

// adds the IMU factors and the prior, evaluated at x (W x 15: PR 6 | VBias 9), to the lidar records (W x 32)
int assemble(const mml_fullwindow* s, const double* records, const double* x, MmlFwEval& e) {
    const int W = s->W, n = s->n;
    e.H.assign((size_t)n * n, 0.0);
    e.g.assign(n, 0.0);
    e.cost = 0;
    for (int f = 0; f < W; ++f) {
        const double* rec = records + 32 * f;
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) e.H[(size_t)(15 * f + a) * n + 15 * f + b] += Hget(rec, a, b);
        for (int a = 0; a < 6; ++a) e.g[15 * f + a] += rec[21 + a];
        e.cost += rec[27];
    }
    for (int f = 1; f < W; ++f) {
        if (!s->have_imu[f]) continue;
        double r[15], J[15 * 30];
        const double* xi = x + 15 * (f - 1);
        const double* xj = x + 15 * f;
        if (!s->U_ok[f]) return MML_ERR_STATE;
        imu_factor_with_U(&s->imu[f], &s->U[225 * (size_t)f], s->gravity, xi, xi + 6, xj, xj + 6, r, J);
        const int base = 15 * (f - 1);  // the 30 columns are exactly the two consecutive frames
        // (each product is summed on its own, then added -- k_fw_eval / k_fw_step's order; mml_fullwindow_marginalize below keeps
        //  ONE running value per element.  Two orders, each held by a byte-equality test against the device: keep them apart)
        for (int a = 0; a < 30; ++a) {
            double ga = 0;
            for (int i = 0; i < 15; ++i) ga += J[i * 30 + a] * r[i];
            e.g[base + a] += ga;
            for (int b = 0; b < 30; ++b) {
                double h = 0;
                for (int i = 0; i < 15; ++i) h += J[i * 30 + a] * J[i * 30 + b];
                e.H[(size_t)(base + a) * n + base + b] += h;
            }
        }
        double c = 0;
        for (int i = 0; i < 15; ++i) c += r[i] * r[i];
        e.cost += 0.5 * c;
    }
    if (s->prior.valid) {
        double r[15];
        prior_residual(s->prior.p, x, r);
        for (int a = 0; a < 15; ++a) {
            double ga = 0;
            for (int i = 0; i < 15; ++i) ga += s->prior.p.J[i * 15 + a] * r[i];
            e.g[a] += ga;
            for (int b = 0; b < 15; ++b) {
                double h = 0;
                for (int i = 0; i < 15; ++i) h += s->prior.p.J[i * 15 + a] * s->prior.p.J[i * 15 + b];
                e.H[(size_t)a * n + b] += h;
            }
        }
        double c = 0;
        for (int i = 0; i < 15; ++i) c += r[i] * r[i];
        e.cost += 0.5 * c;
    }
    return MML_OK;
}

double quad(const mml_fullwindow* s, const std::vector<double>& v) {  // v^T (S H S) v
    const int n = s->n;
    double q = 0;
    for (int a = 0; a < n; ++a) {
        double row = 0;
        for (int b = 0; b < n; ++b) row += s->cur.H[(size_t)a * n + b] * s->scale[b] * v[b];
        q += v[a] * s->scale[a] * row;
    }
    return q;
}

// one proposal: returns 1 when s->xc holds a candidate to evaluate, 0 when the step was invalid (propose again),
// -1 when the minimiser has stopped
int propose(mml_fullwindow* s) {
    const int n = s->n;
    if (s->iter >= s->opts.max_num_iterations || s->radius < 1e-32) return -1;
    s->iter++;
    bool solve_ok = true;
    if (!s->reuse) {
        s->reuse = 1;
        for (int i = 0; i < n; ++i) {
            double d = s->cur.H[(size_t)i * n + i] * s->scale[i] * s->scale[i];
            d = fmin(fmax(d, 1e-6), 1e32);
            s->diag[i] = sqrt(d);
        }
        double gg = 0;
        std::vector<double> sg(n);
        for (int i = 0; i < n; ++i) {
            s->grad[i] = s->cur.g[i] * s->scale[i] / s->diag[i];
            sg[i] = s->grad[i] / s->diag[i];
            gg += s->grad[i] * s->grad[i];
        }
        s->alpha = gg / quad(s, sg);
        solve_ok = false;
        std::vector<double> A((size_t)n * n), b(n);
        while (s->mu < 1.0) {
            for (int a = 0; a < n; ++a) {
                for (int c = 0; c < n; ++c) A[(size_t)a * n + c] = s->cur.H[(size_t)a * n + c] * s->scale[a] * s->scale[c];
                A[(size_t)a * n + a] += s->mu * s->diag[a] * s->diag[a];
                b[a] = s->cur.g[a] * s->scale[a];
            }
            bool ok = cholesky(A.data(), n);
            if (ok) {
                chol_solve_rcp(A.data(), n, b.data());
                for (int a = 0; a < n; ++a)
                    if (!isfinite(b[a])) ok = false;
            }
            if (!ok) {
                s->mu *= 10.0;
                continue;
            }
            for (int a = 0; a < n; ++a) s->gn[a] = -s->diag[a] * b[a];
            solve_ok = true;
            break;
        }
    }
    bool step_valid = solve_ok;
    if (solve_ok) {
        double gradient_norm = 0, gn_norm = 0;
        for (int i = 0; i < n; ++i) {
            gradient_norm += s->grad[i] * s->grad[i];
            gn_norm += s->gn[i] * s->gn[i];
        }
        gradient_norm = sqrt(gradient_norm);
        gn_norm = sqrt(gn_norm);
        if (gn_norm <= s->radius) {
            for (int i = 0; i < n; ++i) s->step[i] = s->gn[i];
            s->dogleg_norm = gn_norm;
        } else if (gradient_norm * s->alpha >= s->radius) {
            for (int i = 0; i < n; ++i) s->step[i] = -(s->radius / gradient_norm) * s->grad[i];
            s->dogleg_norm = s->radius;
        } else {
            double gdot = 0;
            for (int i = 0; i < n; ++i) gdot += s->grad[i] * s->gn[i];
            const double b_dot_a = -s->alpha * gdot;
            const double a_sq = (s->alpha * gradient_norm) * (s->alpha * gradient_norm);
            const double bma_sq = a_sq - 2 * b_dot_a + gn_norm * gn_norm;
            const double c = b_dot_a - a_sq;
            const double d = sqrt(c * c + bma_sq * (s->radius * s->radius - a_sq));
            const double beta = (c <= 0) ? (d - c) / bma_sq : (s->radius * s->radius - a_sq) / (d + c);
            double sn = 0;
            for (int i = 0; i < n; ++i) {
                s->step[i] = (-s->alpha * (1.0 - beta)) * s->grad[i] + beta * s->gn[i];
                sn += s->step[i] * s->step[i];
            }
            s->dogleg_norm = sqrt(sn);
        }
        for (int i = 0; i < n; ++i) s->step[i] /= s->diag[i];
        double sgd = 0;
        for (int i = 0; i < n; ++i) sgd += s->step[i] * s->cur.g[i] * s->scale[i];
        s->model_change = -(sgd + 0.5 * quad(s, s->step));
        if (!(s->model_change > 0.0)) step_valid = false;
    }
    if (!step_valid) {
        if (++s->num_invalid >= 5) {  // HandleInvalidStep: FAILURE, Solver::Solve restores the parameters it was given
            s->x = s->x_init;
            s->termination = 4;
            return -1;
        }
        s->mu *= 10.0;
        s->reuse = 0;
        return 0;
    }
    s->num_invalid = 0;
    double sn = 0;
    for (int i = 0; i < n; ++i) {
        const double delta = s->step[i] * s->scale[i];
        s->xc[i] = s->x[i] + delta;
        sn += delta * delta;
    }
    s->step_norm = sqrt(sn);
    return 1;
}

// after the candidate has been evaluated into s->cand: accept / reject; returns true when the minimiser stops
bool decide(mml_fullwindow* s) {
    const int n = s->n;
    const bool fixed = s->opts.fixed_iterations != 0;
    const double cand = s->cand.cost;
    if (!fixed) {
        if (s->step_norm <= 1e-8 * (s->x_norm + 1e-8)) {
            s->termination = 2;
            return true;
        }
        if (fabs(s->cur.cost - cand) <= 1e-6 * s->cur.cost) {
            s->termination = 3;
            return true;
        }
    }
    const double rel = (s->cur.cost - cand) / s->model_change;
    if (rel > 1e-3) {
        double xn = 0;
        for (int i = 0; i < n; ++i) {
            s->x[i] = s->xc[i];
            xn += s->x[i] * s->x[i];
        }
        s->x_norm = sqrt(xn);
        s->cur = s->cand;
        s->successful++;
        if (!fixed) {
            double gm = 0;
            for (int i = 0; i < n; ++i) gm = fmax(gm, fabs(s->cur.g[i]));
            if (gm <= 1e-10) {
                s->termination = 1;
                return true;
            }
        }
        if (rel < 0.25) s->radius *= 0.5;
        if (rel > 0.75) s->radius = fmax(s->radius, 3.0 * s->dogleg_norm);
        s->mu = fmax(1e-8, 2.0 * s->mu / 10.0);
        s->reuse = 0;
    } else {
        s->radius *= 0.5;
        s->reuse = 1;
    }
    return false;
}

// after the normal equations at x0 have arrived in s->cur: the scaling and the first test; returns true when the minimiser stops
bool begin(mml_fullwindow* s) {
    const int n = s->n;
    s->initial_cost = s->cur.cost;
    double xn = 0;
    for (int i = 0; i < n; ++i) xn += s->x[i] * s->x[i];
    s->x_norm = sqrt(xn);
    for (int i = 0; i < n; ++i) s->scale[i] = 1.0 / (1.0 + sqrt(s->cur.H[(size_t)i * n + i]));  // Jacobi scaling
    if (!s->opts.fixed_iterations) {
        double gm = 0;
        for (int i = 0; i < n; ++i) gm = fmax(gm, fabs(s->cur.g[i]));
        if (gm <= 1e-10) {
            s->termination = 1;
            return true;
        }
    }
    return false;
}

// a round of a replay script (m x 45 band, g, cost) as the dense equations assemble would have left: exact zeros outside the band
void expand_round(const double* rnd, int n, MmlFwEval& e) {
    e.H.assign((size_t)n * n, 0.0);
    for (int a = 0; a < n; ++a)
        for (int c = 0; c < 45; ++c) {
            const int b = 15 * (a / 15 - 1) + c;
            if (b >= 0 && b < n) e.H[(size_t)a * n + b] = rnd[(size_t)a * 45 + c];
        }
    e.g.assign(rnd + (size_t)45 * n, rnd + (size_t)46 * n);
    e.cost = rnd[(size_t)46 * n];
}

}  // namespace

// mml_debug_fw_replay, variant 0: begin / decide / propose in the order mml_fullwindow_step calls them, s->cur / s->cand from the
// script instead of from assemble
void mml_fw_replay_host(const MmlFwReplay& P, int sc) {
    const int W = P.hdr[4 * sc], R = P.hdr[4 * sc + 3], n = 15 * W;
    mml_solve_opts opts;
    memset(&opts, 0, sizeof(opts));
    opts.fixed_iterations = P.hdr[4 * sc + 1];
    opts.max_num_iterations = P.hdr[4 * sc + 2];
    mml_fullwindow* s = mml_fullwindow_create(W, &opts);
    if (!s) return;
    int evaluate = 0;
    for (int r = 0; r < R; ++r) {
        const double* rnd = P.rounds + P.off[sc] + (size_t)r * (46 * (size_t)n + 1);
        int codes[5] = {0, 0, 0, 0, 0}, nprop = 0, decision = 0;
        const bool was_going = !s->done;
        if (r == 0) {
            s->started = 1;
            s->x.assign(P.x0 + 120 * (size_t)sc, P.x0 + 120 * (size_t)sc + n);
            s->x_init = s->x;
            expand_round(rnd, n, s->cur);
            if (begin(s)) s->done = 1;
        } else if (was_going) {
            expand_round(rnd, n, s->cand);
            const MmlFwSnap b{s->mu, s->cur.cost, s->iter, s->reuse, s->termination, s->successful};
            if (decide(s)) s->done = 1;
            decision = mml_fw_decide_code(b, s->termination, s->successful, s->cur.cost, s->model_change);
        }
        while (!s->done) {
            const MmlFwSnap b{s->mu, s->cur.cost, s->iter, s->reuse, s->termination, s->successful};
            const int p = propose(s);
            if (nprop < 5)
                codes[nprop] = mml_fw_propose_code(b, p, s->iter, s->termination, s->mu, opts.max_num_iterations, n, s->grad.data(),
                                                   s->gn.data(), s->alpha, s->radius);
            ++nprop;
            evaluate = p == 1;
            if (p < 0) s->done = 1;
            if (p != 0) break;
        }
        const size_t o = (size_t)P.row[sc] + r;
        double* xc = P.xc + o * 120;
        double* dig = P.dig + o * MML_FW_DIGEST_DOUBLES;
        int* digi = P.digi + o * MML_TR_DIGEST_INTS;
        const int go = s->done ? 0 : 1;
        for (int i = 0; i < n; ++i) xc[i] = (go && evaluate) ? s->xc[i] : s->x[i];  // (what mml_fullwindow_step hands back)
        dig[0] = s->cur.cost;
        dig[1] = s->radius;
        dig[2] = s->mu;
        dig[3] = s->alpha;
        dig[4] = s->dogleg_norm;
        dig[5] = s->model_change;
        dig[6] = s->step_norm;
        dig[7] = s->x_norm;
        for (int i = 0; i < n; ++i) dig[8 + i] = s->x[i];
        digi[0] = s->iter;
        digi[1] = s->successful;
        digi[2] = s->num_invalid;
        digi[3] = s->reuse;
        digi[4] = s->termination;
        digi[5] = go;
        digi[6] = evaluate;
        digi[7] = decision;
        digi[8] = nprop;
        for (int i = 0; i < 5; ++i) digi[9 + i] = i < nprop ? codes[i] : 0;
    }
    mml_fullwindow_destroy(s);
}

extern "C" {

mml_fullwindow* mml_fullwindow_create(int W, const mml_solve_opts* opts) {
    if (W < 1 || W > 8 || !opts) return nullptr;
    mml_fullwindow* s = new mml_fullwindow();
    s->W = W;
    s->n = 15 * W;
    s->opts = *opts;
    s->imu.resize(W);
    s->have_imu.assign(W, 0);
    s->U.assign(225 * (size_t)W, 0.0);
    s->U_ok.assign(W, 0);
    const int n = s->n;
    s->x.assign(n, 0);
    s->xc.assign(n, 0);
    s->scale.assign(n, 1);
    s->diag.assign(n, 1);
    s->grad.assign(n, 0);
    s->gn.assign(n, 0);
    s->step.assign(n, 0);
    return s;
}

void mml_fullwindow_destroy(mml_fullwindow* s) { delete s; }

int mml_fullwindow_set_imu(mml_fullwindow* s, int f, const mml_imu_preint* pre, const double* gravity) {
    if (!s || !pre || !gravity || f < 1 || f >= s->W) return MML_ERR_INVALID;
    s->imu[f] = *pre;
    s->have_imu[f] = 1;
    s->U_ok[f] = imu_sqrt_info(pre, &s->U[225 * (size_t)f]) ? 1 : 0;  // (a covariance that is not positive definite is reported by the solve)
    for (int k = 0; k < 3; ++k) s->gravity[k] = gravity[k];
    return MML_OK;
}

int mml_fullwindow_set_prior(mml_fullwindow* s, const mml_prior* p) {
    if (!s) return MML_ERR_INVALID;
    if (!p) {
        s->prior.valid = false;
        return MML_OK;
    }
    s->prior.valid = true;
    s->prior.p = *p;
    return MML_OK;
}

// Protocol of mml_window_solver_step: `records` are the lidar normal equations (W x 32, from mml_linearize_record /
// the all-gather) evaluated at x_eval (W x 15).  Returns 1 when finished (x_eval holds the solution), 0 when x_eval
// holds the next point to evaluate, < 0 on error.
int mml_fullwindow_step(mml_fullwindow* s, const double* records, double* x_eval) {
    if (!s || !records || !x_eval) return MML_ERR_INVALID;
    const int n = s->n;
    if (s->done) {
        memcpy(x_eval, s->x.data(), sizeof(double) * n);
        return 1;
    }
    if (!s->started) {
        s->started = 1;
        memcpy(s->x.data(), x_eval, sizeof(double) * n);
        s->x_init = s->x;
        int rc = assemble(s, records, s->x.data(), s->cur);
        if (rc != MML_OK) return rc;
        if (begin(s)) {
            s->done = 1;
            return 1;
        }
    } else {
        int rc = assemble(s, records, s->xc.data(), s->cand);
        if (rc != MML_OK) return rc;
        if (decide(s)) {
            s->done = 1;
            memcpy(x_eval, s->x.data(), sizeof(double) * n);
            return 1;
        }
    }
    for (;;) {
        const int p = propose(s);
        if (p < 0) {
            s->done = 1;
            memcpy(x_eval, s->x.data(), sizeof(double) * n);
            return 1;
        }
        if (p == 1) break;
    }
    memcpy(x_eval, s->xc.data(), sizeof(double) * n);
    return 0;
}

// The dense normal equations Ceres would assemble at x: H = sum J^T J (n x n row-major, n = 15 W), g = sum J^T r,
// cost = 1/2 sum r^2 over the lidar blocks (from `records`), the IMU factors and the prior.
int mml_fullwindow_normal_equations(const mml_fullwindow* s, const double* records, const double* x, double* H, double* g,
                                    double* cost) {
    if (!s || !records || !x || !H || !g || !cost) return MML_ERR_INVALID;
    MmlFwEval e;
    int rc = assemble(s, records, x, e);
    if (rc != MML_OK) return rc;
    memcpy(H, e.H.data(), sizeof(double) * e.H.size());
    memcpy(g, e.g.data(), sizeof(double) * e.g.size());
    *cost = e.cost;
    return MML_OK;
}

int mml_fullwindow_summary(const mml_fullwindow* s, mml_solve_summary* out) {
    if (!s || !out) return MML_ERR_INVALID;
    out->iterations = s->iter;
    out->successful = s->successful;
    out->initial_cost = s->initial_cost;
    out->final_cost = s->cur.cost;
    out->termination = s->termination;
    return MML_OK;
}

// MarginalizationInfo::preMarginalize + marginalize (ceresfunc.h:132-228) for the factor set of Estimator.cpp:1453-1546:
// the previous prior (all of its blocks are dropped: it lives on frame 0), the IMU factor between frames 0 and 1, and
// the lidar factors of frame 0 given as their normal equations `lidar_record0` (32 doubles, evaluated WITHOUT a loss
// function at x[0..6)).  x: W x 15 current values.  Result: the prior on (PR, VBias) of frame 1, i.e. of frame 0 once
// the window has slid (:1552-1562).
int mml_fullwindow_marginalize(const mml_fullwindow* s, const double* lidar_record0, const double* x, mml_prior* out) {
    if (!s || !lidar_record0 || !x || !out || s->W < 2 || !s->have_imu[1]) return MML_ERR_INVALID;
    const int N = 30;
    std::vector<double> A((size_t)N * N, 0.0), b(N, 0.0);
    // (every element is ONE running value over prior, IMU and lidar terms -- k_fw_marginalize's order; assemble above sums each
    //  product on its own and adds it.  Two orders, each held by a byte-equality test against the device: keep them apart)
    if (s->prior.valid) {
        double r[15];
        prior_residual(s->prior.p, x, r);
        for (int a = 0; a < 15; ++a) {
            for (int i = 0; i < 15; ++i) b[a] += s->prior.p.J[i * 15 + a] * r[i];
            for (int c = 0; c < 15; ++c)
                for (int i = 0; i < 15; ++i) A[(size_t)a * N + c] += s->prior.p.J[i * 15 + a] * s->prior.p.J[i * 15 + c];
        }
    }
    {
        double r[15], J[15 * 30];
        int rc = s->U_ok[1] ? MML_OK : MML_ERR_STATE;
        if (rc == MML_OK) imu_factor_with_U(&s->imu[1], &s->U[225], s->gravity, x, x + 6, x + 15, x + 21, r, J);
        if (rc != MML_OK) return rc;
        for (int a = 0; a < 30; ++a) {
            for (int i = 0; i < 15; ++i) b[a] += J[i * 30 + a] * r[i];
            for (int c = 0; c < 30; ++c)
                for (int i = 0; i < 15; ++i) A[(size_t)a * N + c] += J[i * 30 + a] * J[i * 30 + c];
        }
    }
    for (int a = 0; a < 6; ++a) {
        for (int c = 0; c < 6; ++c) A[(size_t)a * N + c] += Hget(lidar_record0, a, c);
        b[a] += lidar_record0[21 + a];
    }
    MargWork work;  // the dense tail, shared with the device (marg_dense.h)
    marg_dense(A.data(), b.data(), out->J, out->r0, work);
    memcpy(out->x0, x + 15, sizeof(double) * 15);  // parameter_block_data of the kept blocks = their current values
    return MML_OK;
}

}  // extern "C"
