// fullwindow_internal.h -- the full-window solver handle shared by window_imu.hip (host trust-region loop, IMU factor,
// marginalization) and fullwindow_dev.hip (the same loop resident on the device); its prior is the ABI's mml_prior plus
// a flag.  The dense helpers the host files share (Cholesky, sqrt information) are imu_math.h's; the only functions here belong
// to the replay hook mml_debug_fw_replay (at the end).
#pragma once
#include <math.h>

#include <vector>

#include "../../include/mmloam_hip.h"

struct MmlFwPrior {  // MarginalizationFactor on (para_PR[0], para_VBias[0]) after the address shift (:1552-1562)
    bool valid = false;
    mml_prior p;
};

struct MmlFwEval {  // dense normal equations of the whole window at one x
    std::vector<double> H, g;
    double cost = 0;
};

struct mml_fullwindow {
    int W = 0, n = 0;
    mml_solve_opts opts;
    std::vector<mml_imu_preint> imu;   // imu[f]: between frame f-1 and f (f >= 1)
    std::vector<char> have_imu;
    std::vector<double> U;             // sqrt information of imu[f] (225 each), factored once in mml_fullwindow_set_imu
    std::vector<char> U_ok;
    double gravity[3] = {0, 0, 0};
    MmlFwPrior prior;
    // trust-region state (Ceres 2.1 TRADITIONAL_DOGLEG, same constants as mml_solve / tr_propose / tr_decide)
    std::vector<double> x, xc, x_init, scale, diag, grad, gn, step;
    MmlFwEval cur, cand;
    double radius = 1e4, mu = 1e-8, alpha = 0, dogleg_norm = 0, x_norm = 0, model_change = 0, step_norm = 0;
    int reuse = 0, num_invalid = 0, iter = 0, successful = 0, termination = 0, started = 0, done = 0;
    double initial_cost = 0;
};

// ---- mml_debug_fw_replay (a test hook): what a propose / decide call did, derived from the state before and after it as
// solve.hip's tr_propose_code / tr_decide_code do for the lidar solves; the host replay (window_imu.hip) and the device replay
// (fullwindow_dev.hip) both classify with these.
#if defined(__HIPCC__)
#define MML_FW_HD __host__ __device__
#else
#define MML_FW_HD
#endif

struct MmlFwSnap {  // the state before a call
    double mu, cost;
    int iter, reuse, termination, successful;
};

// p: the return value of the propose call (1 candidate, 0 invalid step, -1 stopped)
MML_FW_HD inline int mml_fw_propose_code(const MmlFwSnap& b, int p, int iter, int termination, double mu, int max_iters, int n,
                                         const double* grad, const double* gn, double alpha, double radius) {
    if (iter == b.iter) return b.iter >= max_iters ? MML_TR_STOP_ITER : MML_TR_STOP_RADIUS;
    const bool failed = termination == 4 && b.termination != 4, invalid = p != 1;
    int k = 0;  // the mu ladder multiplies by 10 and nothing else: counting the same multiplications finds how often it did
    double m = b.mu;
    while (m < mu && k < 64) {
        m *= 10.0;
        ++k;
    }
    const int retries = k - ((invalid && !failed) ? 1 : 0);
    int code;
    if (invalid) {
        double end = b.mu;  // mu when the ladder ended: a solve that failed left it at 1 or above
        for (int i = 0; i < retries; ++i) end *= 10.0;
        code = (!b.reuse && !(end < 1.0)) ? MML_TR_SOLVE_FAILED : MML_TR_MODEL_INVALID;
    } else {
        double gradient_norm = 0, gn_norm = 0;
        for (int i = 0; i < n; ++i) gradient_norm += grad[i] * grad[i];
        for (int i = 0; i < n; ++i) gn_norm += gn[i] * gn[i];
        gradient_norm = sqrt(gradient_norm);
        gn_norm = sqrt(gn_norm);
        if (gn_norm <= radius) {
            code = MML_TR_GAUSS_NEWTON;
        } else if (gradient_norm * alpha >= radius) {
            code = MML_TR_CAUCHY;
        } else {
            double gdot = 0;
            for (int i = 0; i < n; ++i) gdot += grad[i] * gn[i];
            const double b_dot_a = -alpha * gdot;
            const double a_sq = (alpha * gradient_norm) * (alpha * gradient_norm);
            code = (b_dot_a - a_sq <= 0) ? MML_TR_INTERP_NEG : MML_TR_INTERP_POS;
        }
    }
    return code + 16 * retries + (failed ? MML_TR_FAILED : 0);
}

// cost: the current point's after the call (the accepted candidate's when the step was accepted)
MML_FW_HD inline int mml_fw_decide_code(const MmlFwSnap& b, int termination, int successful, double cost, double model_change) {
    if (termination != b.termination)
        return termination == 2 ? MML_TR_D_PARAMETER_TOL : termination == 3 ? MML_TR_D_FUNCTION_TOL : MML_TR_D_GRADIENT_TOL;
    if (successful == b.successful) return MML_TR_D_REJECTED;
    const double rel = (b.cost - cost) / model_change;
    return rel < 0.25 ? MML_TR_D_ACCEPT_SHRINK : rel > 0.75 ? MML_TR_D_ACCEPT_GROW : MML_TR_D_ACCEPT_KEEP;
}

struct MmlFwReplay {  // one call's arguments after the checks; the output pointers are host arrays (variant 0) or device arrays
    int n;
    const int* hdr;
    const double* x0;
    const long long* off;   // per script: its first double in rounds
    const long long* row;   // per script: its first output row
    const double* rounds;
    double* xc;
    double* dig;
    int* digi;
};
// variant 0 of mml_debug_fw_replay: window_imu.hip's propose / decide on script s
void mml_fw_replay_host(const MmlFwReplay& P, int s);
