// fullwindow_dev.hip -- SURVEY.md section 8(f) rank 1 with the trust-region loop resident on the device.
// Estimator::Estimate in full-window mode (mm-loam/src/lio/Estimator.cpp:1226-1254 problem set-up, :1425-1432
// ceres::Solve): W <= 8 frames x [PR 6 | VBias 9], lidar factors of every frame, IMU factors between consecutive frames
// (Cost_NavState_PRV_Bias, ceresfunc.h:321-393), the marginalization prior on frame 0 (ceresfunc.h:244-303).
// window_imu.hip runs this minimisation on the host and comes back to the device for every evaluation of the lidar
// factors; here the Ceres 2.1 TRADITIONAL_DOGLEG iteration is a device-resident state machine advanced by two kernels
// per evaluation, enqueued max_iterations + 1 times without reading anything back (a finished state machine turns the
// remaining launches into no-ops):
//   k_fw_eval   2 W workgroups.  Workgroup f < W: the lidar factors of frame f at the candidate (lidar_eval.h
//               frame_record) -> its 28-value record.  Workgroup W + f: IMU factor f -- residual and Jacobian on one lane
//               (imu_math.h, the code the host solver runs), then the sqrt-information products (imu_math.h imu_whiten,
//               the host's too) and the 30 x 30 J^T J / J^T r of the factor element-parallel; workgroup W: the prior
//               residual and its J^T r.
//   k_fw_step   1 workgroup.  Adds the pieces into the normal equations in the order the host assembly adds them
//               (lidar, IMU f, IMU f + 1, prior).  The 15 W system is block tridiagonal (a factor couples consecutive
//               frames only), so H lives as a band of three 15-column blocks per row, in LDS.  Accept / reject the
//               previous candidate, then Jacobi scaling, the regularised Gauss-Newton step by a right-looking band
//               Cholesky run barrier-free by ONE wavefront (every element receives its subtractions in the order of
//               the dense left-looking host routine; the skipped out-of-band terms are exact zeros there),
//               substitutions with the right-hand side in registers (one lane per row, the pivot handed over by a
//               lane read), dogleg interpolation, the next candidate.  Element-wise work runs on all lanes; sums that
//               Ceres takes sequentially are taken sequentially by one lane each, on different wavefronts at once.
// The trust-region step itself -- everything after the normal equations are assembled, fw_round below -- is bit-identical to
// the host loop's (window_imu.hip: chol_solve_rcp subtracts in the device's order): mml_debug_fw_replay runs both on the same
// scripted equations and tests/test_gpu_fw_tr_kat.py compares every candidate and every state value for equality, over every
// branch and over the sizes at which the band code changes behaviour (n = 15, 30, 45, 75, 120).
// Every kernel carries a window dimension (blockIdx.y = w; parameter block, state machine and output record live in
// arrays of n): mml_fullwindow_solve_batch advances n independent windows with the same launches, mml_fullwindow_solve
// is its n = 1 case.  A window's workgroups touch that window's records only, so its arithmetic does not depend on
// what else is in the batch.
//   k_fw_marginalize   n workgroups.  Frame 0 of window w marginalized into the next prior (mml_fullwindow_marginalize_batch):
//               the loss-free lidar record of frame 0 (frame_record), prior and IMU factor 1 (imu_whiten), the 30 x 30
//               system, then the dense tail of marg_dense.h -- the routine the host function runs -- on one wavefront;
//               bit-identical to the host.
// Host side: the per-call buffers are MmlStaging pairs (mml_mem.h: device array + pinned twin, grow-only), refusals go
// through mml_refuse, and a prior crosses between handle, parameter block and ABI as one mml_prior.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <utility>

#include "fullwindow_internal.h"
#include "imu_math.h"
#include "lidar_eval.h"
#include "marg_dense.h"
#include "mml_internal.h"

// k_fw_step -- the dense 15 W-dimensional trust-region iteration -- keeps 256 threads; the lidar evaluation (k_fw_eval: eval_frame +
// block_reduce28, shared with k_solve / k_linearize / k_window_round so that all of them sum in the same order) runs SOLVE_THREADS.
constexpr int FW_THREADS = 256;
namespace {

constexpr int FW_N = 15 * MAXW;  // 120 parameters at most
constexpr int FW_BW = 45;        // band of H: the blocks blk - 1, blk, blk + 1 of a row
constexpr int FW_LW = 31;        // LDS doubles per row reserved for the Cholesky band (30 used, see lbi())

struct FwDevParams {  // uploaded once per solve
    int W, max_iters, fixed, first, has_prior, pad_[3];
    int have_imu[MAXW];
    double huber, w_tan;
    double gravity[3];
    double pad2_;
    double Tbl[16];
    double x[FW_N];
    mml_prior prior;
    double PP[225];            // prior.J^T prior.J (constant over the solve)
    mml_imu_preint imu[MAXW];  // imu[f]: between frames f - 1 and f
    double U[MAXW][225];       // sqrt information of imu[f], upper triangular
};

#ifdef MML_FW_TIMING
#define FW_T(k) do { __syncthreads(); if (threadIdx.x == 0) { const long long t_ = wall_clock64(); sh.s.ticks[k] += (double)(t_ - sh.s.t_last); sh.s.t_last = t_; } } while (0)
#define FW_TW(k) do { if (threadIdx.x == 0) { const long long t_ = wall_clock64(); sh.s.ticks[k] += (double)(t_ - sh.s.t_last); sh.s.t_last = t_; } } while (0)
#else
#define FW_T(k) do { } while (0)
#define FW_TW(k) do { } while (0)
#endif

struct FwScalars {
    double radius, mu, alpha, dogleg_norm, x_norm, model_change, step_norm, sgd, q, gg, gradient_norm, gn_norm, gdot, sn;
    double cost[2];
    double initial_cost;
    int reuse, num_invalid, iter, successful, termination, cur, flag, evals, go, steps;
#ifdef MML_FW_TIMING
    long long t_last;
    double ticks[16];
#endif
};

struct FwVectors {
    double x[FW_N], xc[FW_N], x_init[FW_N], scale[FW_N], diag[FW_N], grad[FW_N], gn[FW_N], step[FW_N];
    double g[2][FW_N];
};

struct FwGlobal {  // the state machine between the launches
    FwScalars s;
    FwVectors v;
    double Hb[2][FW_N * FW_BW];  // band of the normal equations at x and at the candidate
    // what k_fw_eval leaves for k_fw_step
    double rec[MAXW][28];
    double JJ[MAXW][900], Jr[MAXW][30], rr[MAXW];  // per IMU factor: J^T J, J^T r, r^T r (after the sqrt information)
    double gp[15], rp2;                             // prior: J^T r, r^T r
};

struct FwDevOut {
    double x[FW_N];
    double initial_cost, final_cost;
    int iterations, successful, termination, evaluations, steps, pad_;
#ifdef MML_FW_TIMING
    double ticks[16];
#endif
};

struct FwKernelArgs {
    const FwDevParams* P;  // n parameter blocks
    FwGlobal* G;           // n state machines
    FwDevOut* out;         // n output records
    int* alive;            // alive[r]: windows still going after round r (counted in the rounds the host polls)
    const int* ft_n;
    const MmlLineFactor* lf;
    const MmlPlaneFactor* pf;
    int B, MF, round, poll;
};

__device__ __forceinline__ int band0(int a) { return 15 * (a / 15 - 1); }  // first column of row a's band (may be -15)

// sum_i a[i] * b[i] for i = 0 .. n - 1 in that order, n a multiple of 15; one lane, loads issued 15 at a time
__device__ double ordered_dot(const double* a, const double* b, int n) {
    double s = 0;
    for (int f = 0; f < n; f += 15) {
        double u[15], w[15];
#pragma unroll
        for (int i = 0; i < 15; ++i) {
            u[i] = a[f + i];
            w[i] = b[f + i];
        }
#pragma unroll
        for (int i = 0; i < 15; ++i) s += u[i] * w[i];
    }
    return s;
}

// ---- evaluation ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SOLVE_THREADS) void k_fw_eval(FwKernelArgs A) {
    __shared__ double s_part[SOLVE_WAVES * 28];
    __shared__ double s_x[30];
    __shared__ double s_r[15], s_rs[15];
    __shared__ double s_J[450], s_Js[450];
    const FwDevParams* P = A.P + blockIdx.y;
    FwGlobal* G = A.G + blockIdx.y;
    if (!G->s.go) return;
    const int tid = threadIdx.x, W = P->W, blk = blockIdx.x;
    if (blk >= 2 * W) return;  // the grid covers the largest window of the batch
    if (blk < W) {  // lidar factors of frame blk
        const int b = P->first + blk;
        if (tid < 6) s_x[tid] = G->v.xc[15 * blk + tid];
        __syncthreads();
        frame_record(A.lf, A.pf, A.ft_n, A.B, A.MF, b, s_x, P->Tbl, P->w_tan, P->huber, s_part, G->rec[blk]);
        return;
    }
    const int f = blk - W;
    if (f == 0) {  // MarginalizationFactor on frame 0
        if (!P->has_prior) return;
        if (tid < 15) s_x[tid] = G->v.xc[tid];
        __syncthreads();
        if (tid == 0) prior_residual(P->prior, s_x, s_r);
        __syncthreads();
        if (tid < 15) {
            double p = 0;
            for (int i = 0; i < 15; ++i) p += P->prior.J[i * 15 + tid] * s_r[i];
            G->gp[tid] = p;
        } else if (tid == 64) {
            double c = 0;
            for (int i = 0; i < 15; ++i) c += s_r[i] * s_r[i];
            G->rp2 = c;
        }
        return;
    }
    if (!P->have_imu[f]) return;
    if (tid < 30) s_x[tid] = G->v.xc[15 * (f - 1) + tid];
    __syncthreads();
    if (tid == 0) imu_raw(&P->imu[f], P->gravity, s_x, s_x + 6, s_x + 15, s_x + 21, s_r, s_J);
    __syncthreads();
    for (int o = tid; o < 465; o += SOLVE_THREADS) (o < 450 ? s_Js[o] : s_rs[o - 450]) = imu_whiten(P->U[f], s_J, s_r, o);
    __syncthreads();
    // (each product is summed on its own and handed to k_fw_step, which adds the pieces as the host's assemble does; the
    //  marginalization accumulates prior, IMU and lidar terms in ONE running value -- two orders, each held by a byte-equality test)
    for (int o = tid; o < 931; o += SOLVE_THREADS) {
        if (o < 900) {
            const int a = o / 30, b = o - 30 * a;
            double h = 0;
            for (int i = 0; i < 15; ++i) h += s_Js[i * 30 + a] * s_Js[i * 30 + b];
            G->JJ[f][o] = h;
        } else if (o < 930) {
            const int a = o - 900;
            double h = 0;
            for (int i = 0; i < 15; ++i) h += s_Js[i * 30 + a] * s_rs[i];
            G->Jr[f][a] = h;
        } else {
            double c = 0;
            for (int i = 0; i < 15; ++i) c += s_rs[i] * s_rs[i];
            G->rr[f] = c;
        }
    }
}

// ---- trust-region step -----------------------------------------------------------------------------------------------
struct FwShared {
    double H[FW_N * FW_BW];    // band of the normal equations at the current point
    double big[FW_N * FW_LW];  // the Cholesky band
    FwVectors v;
    double tmp[FW_N], rows[FW_N], bvec[FW_N];
    FwScalars s;
};

// v^T (S H S) v over the band (the out-of-band terms of the dense host loop are exact zeros)
__device__ double fw_quad(FwShared& sh, int n, const double* v) {
    const int tid = threadIdx.x;
    if (tid < n) {
        const int c0 = band0(tid);
        const int lo = max(0, -c0), hi = min(FW_BW, n - c0);
        double row = 0;
        for (int cb = lo; cb < hi; ++cb) row += sh.H[tid * FW_BW + cb] * sh.v.scale[c0 + cb] * v[c0 + cb];
        sh.rows[tid] = v[tid] * sh.v.scale[tid];
        sh.tmp[tid] = row;
    }
    __syncthreads();
    if (tid == 0) sh.s.q = ordered_dot(sh.rows, sh.tmp, n);
    __syncthreads();
    return sh.s.q;
}

// The Cholesky band in LDS: element (i, k), i - 29 <= k <= i, at 29 i + k + 29 -- linear in both indices, so a column
// step addresses everything as (a base that advances by 30 per column) + (a per-lane constant).
__device__ __forceinline__ int lbi(int i, int k) { return 29 * i + k + 29; }

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// the triangle behind a column, enumerated (0,0), (1,0), (1,1), (2,0), ...: entry t is (row, column) relative to j + 1
struct TriTab {
    unsigned char i[448], c[448];
};
constexpr TriTab make_tri_tab() {
    TriTab t{};
    int k = 0;
    for (int i = 0; i < 30; ++i)
        for (int c = 0; c <= i; ++c)
            if (k < 448) {
                t.i[k] = (unsigned char)i;
                t.c[k] = (unsigned char)c;
                ++k;
            }
    return t;
}
__device__ const TriTab kTriTab = make_tri_tab();

// In-place band Cholesky of sh.big (lower) by wavefront 0, then L L^T z = bvec, z -> bvec.  Returns 0 when the matrix is
// not positive definite or the solution is not finite.  Right-looking: column j is scaled, then the (at most 29 x 29)
// triangle behind it is updated, 64 elements at a time; no workgroup barrier inside.
__device__ int fw_factor_solve(FwShared& sh, int n) {
    const int lane = threadIdx.x;  // called by threads 0 .. 63
    double* L = sh.big;
    int pi[7], oa[7], ob[7], oe[7];  // the triangle entries this lane owns and their offsets from the column base
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const int t = lane + 64 * k;
        const int ii = kTriTab.i[t], cc = kTriTab.c[t];
        pi[k] = ii;
        oa[k] = 58 + 29 * ii;        // L[j + 1 + ii][j]
        ob[k] = 58 + 29 * cc;        // L[j + 1 + cc][j]
        oe[k] = 59 + 29 * ii + cc;   // A[j + 1 + ii][j + 1 + cc]
    }
    int ok = 1;
    FW_TW(7);
#ifdef MML_FW_TIMING
    const long long c0_ = clock64();
#endif
    double d0 = L[29];
    for (int j = 0; j < n; ++j) {
        double* Lj = L + 30 * j;  // Lj[29] = (j, j), Lj[58 + 29 l] = (j + 1 + l, j)
        const int jend = min(n, 15 * (j / 15 + 2)), m = jend - j - 1;
        const double col = Lj[lane < m ? 58 + 29 * lane : 29];  // requested before the square root is taken
        if (!(d0 > 0.0) || !isfinite(d0)) {  // the same value in every lane
            ok = 0;
            break;
        }
        const double d = sqrt(d0);
        if (lane < m) Lj[58 + 29 * lane] = col / d;
        if (lane == 0) Lj[29] = d;
        wave_sync();
        // all loads of the triangle first, then the arithmetic, then the stores: one LDS round trip per column
        double ua[7], ub[7], ue[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const bool act = pi[k] < m;
            ua[k] = Lj[act ? oa[k] : 29];
            ub[k] = Lj[act ? ob[k] : 29];
            ue[k] = Lj[act ? oe[k] : 29];
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) ue[k] -= ua[k] * ub[k];
        d0 = readlane_f64(ue[0], 0);  // element (j + 1, j + 1): the next pivot, without waiting for the store below
#pragma unroll
        for (int k = 0; k < 7; ++k)
            if (pi[k] < m) Lj[oe[k]] = ue[k];
        wave_sync();
    }
    FW_TW(8);
#ifdef MML_FW_TIMING
    if (threadIdx.x == 0) sh.s.ticks[11] += (double)(clock64() - c0_);
#endif
    if (!ok) return 0;
    // forward substitution: lane l carries the right-hand sides of rows l and l + 64 (never inside one band at once) and
    // the reciprocals of their pivots; the element of L a step needs is requested one step ahead
    double s0 = lane < n ? sh.bvec[lane] : 0.0, s1 = lane + 64 < n ? sh.bvec[lane + 64] : 0.0;
    const double r0 = lane < n ? 1.0 / L[lbi(lane, lane)] : 0.0, r1 = lane + 64 < n ? 1.0 / L[lbi(lane + 64, lane + 64)] : 0.0;
    auto fwd_row = [&](int k) { return (k + 1) + ((lane - (k + 1)) & 63); };  // the row >= k + 1 this lane carries
    double lnext = 0.0;
    {
        const int i = fwd_row(0);
        lnext = L[i < min(n, 30) ? lbi(i, 0) : 29];
    }
    for (int k = 0; k < n; ++k) {
        const double lcur = lnext;
        const int i = fwd_row(k), kend = min(n, 15 * (k / 15 + 2));
        if (k + 1 < n) {
            const int i2 = fwd_row(k + 1), kend2 = min(n, 15 * ((k + 1) / 15 + 2));
            lnext = L[i2 < kend2 ? lbi(i2, k + 1) : 29];
        }
        const double sk = readlane_f64((k & 64) ? s1 : s0, k & 63);
        const double yk = sk * readlane_f64((k & 64) ? r1 : r0, k & 63);
        const double u = lcur * yk;
        const bool act = i < kend, hi = (i & 64) != 0, own = lane == (k & 63), khi = (k & 64) != 0;
        s0 = (own && !khi) ? yk : ((act && !hi) ? s0 - u : s0);
        s1 = (own && khi) ? yk : ((act && hi) ? s1 - u : s1);
    }
    FW_TW(9);
    // backward substitution (the columns become known from the last one down)
    auto bwd_row = [&](int k) { return (k - 1) - (((k - 1) - lane) & 63); };  // the row <= k - 1 this lane carries
    {
        const int k = n - 1, i = bwd_row(k);
        lnext = L[(i >= max(0, band0(k)) && k >= 1) ? lbi(k, i) : 29];
    }
    for (int k = n - 1; k >= 0; --k) {
        const double lcur = lnext;
        const int i = bwd_row(k), k0 = max(0, band0(k));
        if (k >= 1) {
            const int k2 = k - 1, i2 = bwd_row(k2);
            lnext = L[(i2 >= max(0, band0(k2)) && k2 >= 1) ? lbi(k2, i2) : 29];
        }
        const double sk = readlane_f64((k & 64) ? s1 : s0, k & 63);
        const double zk = sk * readlane_f64((k & 64) ? r1 : r0, k & 63);
        const double u = lcur * zk;
        const bool act = i >= k0 && k >= 1, hi = (i & 64) != 0, own = lane == (k & 63), khi = (k & 64) != 0;
        s0 = (own && !khi) ? zk : ((act && !hi) ? s0 - u : s0);
        s1 = (own && khi) ? zk : ((act && hi) ? s1 - u : s1);
    }
    FW_TW(10);
    int bad = 0;
    if (lane < n) {
        sh.bvec[lane] = s0;
        bad |= !isfinite(s0);
    }
    if (lane + 64 < n) {
        sh.bvec[lane + 64] = s1;
        bad |= !isfinite(s1);
    }
    return __any(bad) ? 0 : 1;
}

// One proposal (mml_fullwindow_step's propose): 1 = sh.v.xc holds a candidate, 0 = invalid step (propose again),
// -1 = the minimiser has stopped.  The return value is the same in every thread.
__device__ int fw_propose(int max_iters, FwShared& sh, int n) {
    const int tid = threadIdx.x;
    FwScalars& S = sh.s;
    FwVectors& V = sh.v;
    __syncthreads();
    if (S.iter >= max_iters || S.radius < 1e-32) return -1;
    const int reuse = S.reuse;
    const double* g = V.g[S.cur];
    __syncthreads();
    if (tid == 0) S.iter++;
    bool solve_ok = true;
    if (!reuse) {
        if (tid == 0) S.reuse = 1;
        if (tid < n) {
            double d = sh.H[tid * FW_BW + (tid - band0(tid))] * V.scale[tid] * V.scale[tid];
            d = fmin(fmax(d, 1e-6), 1e32);
            const double dg = sqrt(d);
            V.diag[tid] = dg;
            const double gr = g[tid] * V.scale[tid] / dg;
            V.grad[tid] = gr;
            sh.bvec[tid] = gr / dg;  // the Cauchy direction in the scaled space
        }
        __syncthreads();
        if (tid == 64) S.gg = ordered_dot(V.grad, V.grad, n);
        const double q = fw_quad(sh, n, sh.bvec);
        if (tid == 0) {
            S.alpha = S.gg / q;
            S.gradient_norm = sqrt(S.gg);
        }
        FW_T(2);
        solve_ok = false;
        for (;;) {
            __syncthreads();
            const double mu = S.mu;
            if (!(mu < 1.0)) break;
            for (int o = tid; o < n * 30; o += FW_THREADS) {
                const int i = o / 30, k = band0(i) + (o - 30 * i);
                if (k < 0 || k > i) continue;
                double a = sh.H[i * FW_BW + (k - band0(i))] * V.scale[i] * V.scale[k];
                if (k == i) a += mu * V.diag[i] * V.diag[i];
                sh.big[lbi(i, k)] = a;
            }
            if (tid < n) sh.bvec[tid] = g[tid] * V.scale[tid];
            __syncthreads();
            FW_T(3);
            if (tid < 64) {
                const int ok = fw_factor_solve(sh, n);
                if (tid == 0) S.flag = ok;
            }
            __syncthreads();
            FW_T(4);
            if (!S.flag) {
                __syncthreads();
                if (tid == 0) S.mu = mu * 10.0;
                continue;
            }
            if (tid < n) V.gn[tid] = -V.diag[tid] * sh.bvec[tid];
            solve_ok = true;
            break;
        }
        __syncthreads();
    }
    bool step_valid = solve_ok;
    if (solve_ok) {
        // the three sums of the dogleg on three wavefronts
        if (tid == 0) S.gn_norm = sqrt(ordered_dot(V.gn, V.gn, n));
        if (tid == 64) S.gdot = ordered_dot(V.grad, V.gn, n);
        __syncthreads();
        const double gradient_norm = S.gradient_norm, gn_norm = S.gn_norm, radius = S.radius, alpha = S.alpha;
        int branch;
        double beta = 0;
        if (gn_norm <= radius) {
            branch = 0;
            if (tid < n) V.step[tid] = V.gn[tid];
        } else if (gradient_norm * alpha >= radius) {
            branch = 1;
            if (tid < n) V.step[tid] = -(radius / gradient_norm) * V.grad[tid];
        } else {
            branch = 2;
            const double b_dot_a = -alpha * S.gdot;
            const double a_sq = (alpha * gradient_norm) * (alpha * gradient_norm);
            const double bma_sq = a_sq - 2 * b_dot_a + gn_norm * gn_norm;
            const double c = b_dot_a - a_sq;
            const double d = sqrt(c * c + bma_sq * (radius * radius - a_sq));
            beta = (c <= 0) ? (d - c) / bma_sq : (radius * radius - a_sq) / (d + c);
            if (tid < n) V.step[tid] = (-alpha * (1.0 - beta)) * V.grad[tid] + beta * V.gn[tid];
        }
        __syncthreads();
        if (tid == 128 && branch == 2) S.sn = ordered_dot(V.step, V.step, n);
        __syncthreads();
        if (tid < n) {
            const double st = V.step[tid] / V.diag[tid];
            V.step[tid] = st;
            sh.bvec[tid] = st * g[tid];
        }
        __syncthreads();
        if (tid == 64) S.sgd = ordered_dot(sh.bvec, V.scale, n);
        if (tid == 0) S.dogleg_norm = branch == 0 ? gn_norm : (branch == 1 ? radius : sqrt(S.sn));
        const double q = fw_quad(sh, n, V.step);
        const double model_change = -(S.sgd + 0.5 * q);
        if (!(model_change > 0.0)) step_valid = false;
        __syncthreads();
        if (tid == 0) S.model_change = model_change;
        FW_T(5);
    }
    if (!step_valid) {
        __syncthreads();
        if (tid == 0) {
            if (++S.num_invalid >= 5) {  // HandleInvalidStep: FAILURE, the parameters go back as they came in
                S.termination = 4;
                S.flag = -1;
            } else {
                S.mu *= 10.0;
                S.reuse = 0;
                S.flag = 0;
            }
        }
        __syncthreads();
        const int flag = S.flag;
        if (flag < 0 && tid < n) V.x[tid] = V.x_init[tid];
        return flag;
    }
    if (tid < n) {
        const double delta = V.step[tid] * V.scale[tid];
        V.xc[tid] = V.x[tid] + delta;
        sh.bvec[tid] = delta;
    }
    __syncthreads();
    if (tid == 0) {
        S.num_invalid = 0;
        S.step_norm = sqrt(ordered_dot(sh.bvec, sh.bvec, n));
    }
    __syncthreads();
    FW_T(6);
    return 1;
}

// accept / reject after the candidate was evaluated into slot 1 - cur; true when the minimiser stops.  On acceptance
// sh.H (holding the candidate's band) becomes the current band; on rejection the current band is read back from Hb (the two
// slots of FwGlobal::Hb).
__device__ bool fw_decide(bool fixed, const double (*Hb)[FW_N * FW_BW], FwShared& sh, int n) {
    FwScalars& S = sh.s;
    FwVectors& V = sh.v;
    const int tid = threadIdx.x;
    __syncthreads();
    const double cur = S.cost[S.cur], cand = S.cost[1 - S.cur];
    if (!fixed) {
        int stop = 0, term = 0;
        if (S.step_norm <= 1e-8 * (S.x_norm + 1e-8)) {
            term = 2;
            stop = 1;
        } else if (fabs(cur - cand) <= 1e-6 * cur) {
            term = 3;
            stop = 1;
        }
        if (stop) {
            __syncthreads();
            if (tid == 0) S.termination = term;
            return true;
        }
    }
    const double rel = (cur - cand) / S.model_change;
    const int cur_slot = S.cur;
    __syncthreads();
    if (rel > 1e-3) {
        if (tid < n) V.x[tid] = V.xc[tid];
        __syncthreads();
        if (tid == 0) {
            S.x_norm = sqrt(ordered_dot(V.x, V.x, n));
            S.cur = 1 - cur_slot;
            S.successful++;
            int stop = 0;
            if (!fixed) {
                double gm = 0;
                for (int i = 0; i < n; ++i) gm = fmax(gm, fabs(V.g[1 - cur_slot][i]));
                if (gm <= 1e-10) {
                    S.termination = 1;
                    stop = 1;
                }
            }
            if (!stop) {
                if (rel < 0.25) S.radius *= 0.5;
                if (rel > 0.75) S.radius = fmax(S.radius, 3.0 * S.dogleg_norm);
                S.mu = fmax(1e-8, 2.0 * S.mu / 10.0);
                S.reuse = 0;
            }
            S.flag = stop;
        }
    } else {
        for (int o = tid; o < n * FW_BW; o += FW_THREADS) sh.H[o] = Hb[cur_slot][o];
        if (tid == 0) {
            S.radius *= 0.5;
            S.reuse = 1;
            S.flag = 0;
        }
    }
    __syncthreads();
    return S.flag != 0;
}

struct FwTrace {  // what a round did, for mml_debug_fw_replay (in LDS; the solve passes none)
    int decide, nprop, codes[5], evaluate;
};

// One round of the state machine once the normal equations have been assembled into sh.H / Hb[e] / V.g[e] / S.cost[e]: round 0
// initialises (Jacobi scaling, the gradient tolerance), a later round accepts or rejects the candidate; then proposals until a
// candidate needs evaluating or the minimiser stops.  Returns true when it has stopped (the same value in every thread).
// TRACE: the replay's build, which classifies every call into tr; the solve's build carries none of it.
template <bool TRACE>
__device__ __forceinline__ bool fw_round(bool first, int max_iters, bool fixed, const double (*Hb)[FW_N * FW_BW], FwShared& sh, int n, FwTrace* tr) {
    FwScalars& S = sh.s;
    FwVectors& V = sh.v;
    const int tid = threadIdx.x;
    bool done;
    MmlFwSnap snap;  // (thread 0's, when there is a trace)
    if (first) {
        if (tid < n) V.scale[tid] = 1.0 / (1.0 + sqrt(sh.H[tid * FW_BW + (tid - band0(tid))]));  // Jacobi scaling
        if (tid == 0) {
            S.initial_cost = S.cost[0];
            S.x_norm = sqrt(ordered_dot(V.x, V.x, n));
            S.flag = 0;
            if (!fixed) {
                double gm = 0;
                for (int i = 0; i < n; ++i) gm = fmax(gm, fabs(V.g[0][i]));
                if (gm <= 1e-10) {
                    S.termination = 1;
                    S.flag = 1;
                }
            }
        }
        __syncthreads();
        done = S.flag != 0;
    } else {
        if (TRACE && tid == 0) snap = MmlFwSnap{S.mu, S.cost[S.cur], S.iter, S.reuse, S.termination, S.successful};
        done = fw_decide(fixed, Hb, sh, n);
        if (TRACE) {
            __syncthreads();
            if (tid == 0) tr->decide = mml_fw_decide_code(snap, S.termination, S.successful, S.cost[S.cur], S.model_change);
        }
    }
    FW_T(1);
    if (!done) {
        int p;
        do {
            if (TRACE) {
                __syncthreads();
                if (tid == 0) snap = MmlFwSnap{S.mu, S.cost[S.cur], S.iter, S.reuse, S.termination, S.successful};
            }
            p = fw_propose(max_iters, sh, n);
            if (TRACE) {
                __syncthreads();
                if (tid == 0) {
                    if (tr->nprop < 5)
                        tr->codes[tr->nprop] = mml_fw_propose_code(snap, p, S.iter, S.termination, S.mu, max_iters, n, V.grad, V.gn, S.alpha, S.radius);
                    tr->nprop++;
                    tr->evaluate = p == 1;
                }
            }
        } while (p == 0);
        if (p < 0) done = true;
    }
    __syncthreads();
    return done;
}

__global__ __launch_bounds__(FW_THREADS) void k_fw_step(FwKernelArgs A) {
    __shared__ FwShared sh;
    const FwDevParams* P = A.P + blockIdx.y;
    FwGlobal* G = A.G + blockIdx.y;
    FwDevOut* out = A.out + blockIdx.y;
    const int tid = threadIdx.x, W = P->W, n = 15 * W;
    if (!G->s.go) return;  // finished: nothing of this window is written any more
    const bool last = A.round >= P->max_iters;  // this window's own last round
    FwScalars& S = sh.s;
    FwVectors& V = sh.v;
    {
        const double* src = reinterpret_cast<const double*>(&G->v);
        double* dst = reinterpret_cast<double*>(&V);
        for (int i = tid; i < (int)(sizeof(FwVectors) / sizeof(double)); i += FW_THREADS) dst[i] = src[i];
        if (tid == 0) S = G->s;
    }
    __syncthreads();
#ifdef MML_FW_TIMING
    if (tid == 0) S.t_last = wall_clock64();
#endif
    // the normal equations at the candidate, every element summed in the order of the host assembly
    const int e = A.round == 0 ? 0 : 1 - S.cur;
    // (every load is issued whether its term exists or not -- from a clamped address, the value then replaced by +0.0,
    //  which leaves the sum unchanged -- so the loads of several elements are in flight together)
    const int has_prior = P->has_prior;
    unsigned have = 0;  // bit f: IMU factor f present
    for (int f = 1; f < W; ++f) have |= P->have_imu[f] ? 1u << f : 0u;
#pragma unroll 4
    for (int o = tid; o < n * FW_BW; o += FW_THREADS) {
        const int a = o / FW_BW, F = a / 15, la = a - 15 * F;
        const int b = 15 * (F - 1) + (o - FW_BW * a);
        const bool inb = b >= 0 && b < n;
        const int bb = inb ? b : a, Gb = bb / 15, lb = bb - 15 * Gb;
        const bool dg = Gb == F, up = Gb == F + 1, lo = Gb == F - 1;
        const int F1 = min(F + 1, MAXW - 1);
        const bool use_l = inb && dg && la < 6 && lb < 6;
        const bool use_1 = inb && (dg || lo) && ((have >> F) & 1u);        // IMU factor F (frames F - 1, F)
        const bool use_2 = inb && (dg || up) && ((have >> (F + 1)) & 1u);  // IMU factor F + 1 (frames F, F + 1)
        const bool use_p = inb && dg && F == 0 && has_prior;
        const int la6 = min(la, 5), lb6 = min(lb, 5);
        const double v_l = G->rec[F][la6 <= lb6 ? tri(la6, lb6) : tri(lb6, la6)];
        const double v_1 = G->JJ[F][(15 + la) * 30 + (dg ? 15 + lb : lb)];
        const double v_2 = G->JJ[F1][la * 30 + (dg ? lb : 15 + lb)];
        const double v_p = P->PP[la * 15 + lb];
        double h = 0.0;
        h += use_l ? v_l : 0.0;
        h += use_1 ? v_1 : 0.0;
        h += use_2 ? v_2 : 0.0;
        h += use_p ? v_p : 0.0;
        sh.H[o] = h;
        G->Hb[e][o] = h;
    }
    if (tid < n) {
        const int F = tid / 15, la = tid - 15 * F;
        double g = 0.0;
        if (la < 6) g += G->rec[F][21 + la];
        if (F >= 1 && P->have_imu[F]) g += G->Jr[F][15 + la];
        if (F + 1 < W && P->have_imu[F + 1]) g += G->Jr[F + 1][la];
        if (F == 0 && P->has_prior) g += G->gp[la];
        V.g[e][tid] = g;
    }
    if (tid == FW_THREADS - 1) {
        double cost = 0;
        for (int f = 0; f < W; ++f) cost += G->rec[f][27];
        for (int f = 1; f < W; ++f)
            if (P->have_imu[f]) cost += 0.5 * G->rr[f];
        if (P->has_prior) cost += 0.5 * G->rp2;
        S.cost[e] = cost;
        S.evals++;
        S.steps++;
    }
    __syncthreads();
    FW_T(0);
    const bool done = fw_round<false>(A.round == 0, P->max_iters, P->fixed != 0, G->Hb, sh, n, nullptr);
    if (tid == 0) {
        if (done) S.go = 0;
        G->s = S;
    }
    {
        double* dst = reinterpret_cast<double*>(&G->v);
        const double* src = reinterpret_cast<const double*>(&V);
        for (int i = tid; i < (int)(sizeof(FwVectors) / sizeof(double)); i += FW_THREADS) dst[i] = src[i];
    }
    if (done || last) {
        if (tid < n) out->x[tid] = V.x[tid];
        if (tid == 0) {
            out->initial_cost = S.initial_cost;
            out->final_cost = S.cost[S.cur];
            out->iterations = S.iter;
            out->successful = S.successful;
            out->termination = S.termination;
            out->evaluations = S.evals;
            out->steps = S.steps;
#ifdef MML_FW_TIMING
            for (int k = 0; k < 16; ++k) out->ticks[k] = S.ticks[k];
#endif
        }
    }
    // the early-out of the enqueue loop: one count for the whole batch, read back once per chunk
    if (A.poll && !done && tid == 0) atomicAdd(&A.alive[A.round], 1);
}

__global__ void k_fw_init(const FwDevParams* P, FwGlobal* G, int* alive, int rounds) {
    P += blockIdx.y;
    G += blockIdx.y;
    const int tid = threadIdx.x, n = 15 * P->W;
    if (blockIdx.y == 0)
        for (int r = tid; r < rounds; r += blockDim.x) alive[r] = 0;
    if (tid < n) G->v.x[tid] = G->v.xc[tid] = G->v.x_init[tid] = P->x[tid];
    if (tid == 0) {
        FwScalars s;
        memset(&s, 0, sizeof(s));
        s.radius = 1e4;
        s.mu = 1e-8;
        s.go = 1;
        G->s = s;
    }
}

// the 32-double record of every window's frame 0 at the returned x (k_linearize's record: what mml_linearize_window(first, 1, ...)
// hands out and mml_fullwindow_marginalize consumes), workgroup w for window w
__global__ __launch_bounds__(SOLVE_THREADS) void k_fw_record0(FwKernelArgs A, const double* stats, double* record) {
    __shared__ double s_part[SOLVE_WAVES * 28];
    __shared__ double s_out[28];
    const FwDevParams* P = A.P + blockIdx.x;
    const int b = P->first;
    record += 32 * (size_t)blockIdx.x;
    frame_record(A.lf, A.pf, A.ft_n, A.B, A.MF, b, A.out[blockIdx.x].x, P->Tbl, P->w_tan, P->huber, s_part, s_out);
    if (threadIdx.x < 28) record[threadIdx.x] = s_out[threadIdx.x];
    if (threadIdx.x == 0) {
        record[28] = stats[16 * b + 2];
        record[29] = stats[16 * b + 3];
        record[30] = 0;
        record[31] = 0;
    }
}

// ---- marginalization of frame 0 (mml_fullwindow_marginalize on the device) ------------------------------------------------
struct FwMargParams {  // one window's inputs, about 8 KB (the 49 KB FwDevParams carries the whole window)
    int first, has_prior, pad_[2];
    double w_tan, huber;  // huber: always 0 -- the reference stores these factors without a loss function
    double gravity[3];
    double pad2_;
    double Tbl[16];
    double x[30];  // frames 0 and 1
    mml_prior prior;
    mml_imu_preint imu;  // between frames 0 and 1
    double U[225];       // its sqrt information
};

struct FwMargShared {
    double A[900], b[30];
    MargWork work;
    double x[30];
    double rec[28];
    double rp[15], r[15], rs[15];  // prior residual; IMU residual before / after the sqrt information
    double J[450], Js[450];        // IMU Jacobian before / after
    double part[SOLVE_WAVES * 28];
};

// Workgroup w: MarginalizationInfo::preMarginalize + marginalize for window w.  The loss-free lidar record of frame 0 as
// k_fw_record0 / k_linearize form it, the prior residual and the IMU factor 0-1 on one lane each (imu_math.h), A and b
// element-parallel with every element accumulated in the order of the host loop (prior terms, IMU terms, lidar value),
// then the dense tail (marg_dense.h) on wavefront 0.
__global__ __launch_bounds__(SOLVE_THREADS) void k_fw_marginalize(const FwMargParams* Pn, mml_prior* outn, const int* ft_n,
                                                                 const MmlLineFactor* lf, const MmlPlaneFactor* pf, int B, int MF) {
    __shared__ FwMargShared sh;
    const FwMargParams* P = Pn + blockIdx.x;
    mml_prior* out = outn + blockIdx.x;
    const int tid = threadIdx.x, b0 = P->first, has_prior = P->has_prior;
    if (tid < 30) sh.x[tid] = P->x[tid];
    __syncthreads();
    frame_record(lf, pf, ft_n, B, MF, b0, sh.x, P->Tbl, P->w_tan, P->huber, sh.part, sh.rec);
    if (tid == 0 && has_prior) prior_residual(P->prior, sh.x, sh.rp);
    if (tid == 64) imu_raw(&P->imu, P->gravity, sh.x, sh.x + 6, sh.x + 15, sh.x + 21, sh.r, sh.J);
    __syncthreads();
    for (int o = tid; o < 465; o += SOLVE_THREADS) (o < 450 ? sh.Js[o] : sh.rs[o - 450]) = imu_whiten(P->U, sh.J, sh.r, o);
    __syncthreads();
    // (prior, IMU and lidar terms go into ONE running value, as in the host's mml_fullwindow_marginalize; k_fw_eval / assemble form
    //  each product as a sum of its own and add it afterwards -- two orders, each held by a byte-equality test: keep them apart)
    for (int o = tid; o < 930; o += SOLVE_THREADS) {
        double h = 0.0;
        if (o < 900) {
            const int a = o / 30, c = o - 30 * a;
            if (has_prior && a < 15 && c < 15)
                for (int i = 0; i < 15; ++i) h += P->prior.J[i * 15 + a] * P->prior.J[i * 15 + c];
            for (int i = 0; i < 15; ++i) h += sh.Js[i * 30 + a] * sh.Js[i * 30 + c];
            if (a < 6 && c < 6) h += Hget(sh.rec, a, c);
            sh.A[o] = h;
        } else {
            const int a = o - 900;
            if (has_prior && a < 15)
                for (int i = 0; i < 15; ++i) h += P->prior.J[i * 15 + a] * sh.rp[i];
            for (int i = 0; i < 15; ++i) h += sh.Js[i * 30 + a] * sh.rs[i];
            if (a < 6) h += sh.rec[21 + a];
            sh.b[a] = h;
        }
    }
    __syncthreads();
    if (tid < 64) marg_dense(sh.A, sh.b, out->J, out->r0, sh.work);
    else if (tid < 64 + 15) out->x0[tid - 64] = sh.x[15 + tid - 64];  // parameter_block_data of the kept blocks
}

// test hook (mml_marginalize_dense): the dense tail alone, one workgroup of one wavefront per caller-supplied system
__global__ __launch_bounds__(64) void k_marg_dense(const double* A, const double* b, double* J, double* r0) {
    __shared__ double s_A[900], s_b[30];
    __shared__ MargWork s_work;
    const size_t w = blockIdx.x;
    for (int o = threadIdx.x; o < 900; o += 64) s_A[o] = A[900 * w + o];
    if (threadIdx.x < 30) s_b[threadIdx.x] = b[30 * w + threadIdx.x];
    __syncthreads();
    marg_dense(s_A, s_b, J + 225 * w, r0 + 15 * w, s_work);
}

// test hook (mml_debug_fw_replay, variant 1): workgroup s runs fw_round on the rounds of script s, the normal equations taken from
// the script where k_fw_step assembles them.  The state stays in LDS over the rounds (k_fw_step carries it through FwGlobal, a
// copy); Hb: the script's two band slots, 2 x FW_N x FW_BW doubles.
__global__ __launch_bounds__(FW_THREADS) void k_fw_replay(MmlFwReplay P, double* Hb_all) {
    __shared__ FwShared sh;
    __shared__ FwTrace tr;
    const int tid = threadIdx.x, sc = blockIdx.x;
    const int W = P.hdr[4 * sc], fixed = P.hdr[4 * sc + 1], max_iters = P.hdr[4 * sc + 2], R = P.hdr[4 * sc + 3], n = 15 * W;
    double (*Hb)[FW_N * FW_BW] = reinterpret_cast<double (*)[FW_N * FW_BW]>(Hb_all + (size_t)sc * 2 * FW_N * FW_BW);
    FwScalars& S = sh.s;
    FwVectors& V = sh.v;
    {  // k_fw_init
        double* dst = reinterpret_cast<double*>(&V);
        for (int i = tid; i < (int)(sizeof(FwVectors) / sizeof(double)); i += FW_THREADS) dst[i] = 0.0;
        __syncthreads();
        if (tid < n) V.x[tid] = V.xc[tid] = V.x_init[tid] = P.x0[(size_t)sc * FW_N + tid];
        if (tid == 0) {
            FwScalars s;
            memset(&s, 0, sizeof(s));
            s.radius = 1e4;
            s.mu = 1e-8;
            s.go = 1;
            S = s;
            tr.evaluate = 0;
        }
    }
    __syncthreads();
    for (int r = 0; r < R; ++r) {
        const double* rnd = P.rounds + P.off[sc] + (size_t)r * (46 * (size_t)n + 1);
        if (tid == 0) {
            tr.decide = tr.nprop = 0;
            for (int i = 0; i < 5; ++i) tr.codes[i] = 0;
        }
        __syncthreads();
        if (S.go) {  // (uniform: nobody writes the state between the barriers around this read)
            const int e = r == 0 ? 0 : 1 - S.cur;
            for (int o = tid; o < n * FW_BW; o += FW_THREADS) {
                const int a = o / FW_BW, b = band0(a) + (o - FW_BW * a);
                const double h = (b >= 0 && b < n) ? rnd[o] : 0.0;
                sh.H[o] = h;
                Hb[e][o] = h;
            }
            if (tid < n) V.g[e][tid] = rnd[(size_t)FW_BW * n + tid];
            if (tid == FW_THREADS - 1) S.cost[e] = rnd[(size_t)(FW_BW + 1) * n];
            __syncthreads();
            const bool done = fw_round<true>(r == 0, max_iters, fixed != 0, Hb, sh, n, &tr);
            if (done && tid == 0) S.go = 0;
            __syncthreads();
        }
        const size_t o = (size_t)P.row[sc] + r;
        const bool cand = S.go && tr.evaluate;
        if (tid < n) {
            P.xc[o * FW_N + tid] = cand ? V.xc[tid] : V.x[tid];
            P.dig[o * MML_FW_DIGEST_DOUBLES + 8 + tid] = V.x[tid];
        }
        if (tid == 0) {
            double* dig = P.dig + o * MML_FW_DIGEST_DOUBLES;
            int* digi = P.digi + o * MML_TR_DIGEST_INTS;
            dig[0] = S.cost[S.cur];
            dig[1] = S.radius;
            dig[2] = S.mu;
            dig[3] = S.alpha;
            dig[4] = S.dogleg_norm;
            dig[5] = S.model_change;
            dig[6] = S.step_norm;
            dig[7] = S.x_norm;
            digi[0] = S.iter;
            digi[1] = S.successful;
            digi[2] = S.num_invalid;
            digi[3] = S.reuse;
            digi[4] = S.termination;
            digi[5] = S.go;
            digi[6] = tr.evaluate;
            digi[7] = tr.decide;
            digi[8] = tr.nprop;
            for (int i = 0; i < 5; ++i) digi[9 + i] = i < tr.nprop ? tr.codes[i] : 0;
        }
        __syncthreads();
    }
}

constexpr int FW_MAX_ROUNDS = 1001;  // max_num_iterations <= 1000

}  // namespace

struct MmlFwDev {  // every buffer holds the largest batch its call has seen; the two sets grow independently
    MmlStaging<FwDevParams> par;
    MmlStaging<FwGlobal, false> state;
    MmlStaging<FwDevOut> out;
    MmlStaging<int, false> alive;  // FW_MAX_ROUNDS
    MmlStaging<double> rec0;       // 32 per window
    // mml_fullwindow_marginalize_batch
    MmlStaging<FwMargParams> mpar;
    MmlStaging<mml_prior> mout;
    ~MmlFwDev() {
        par.release();
        state.release();
        out.release();
        alive.release();
        rec0.release();
        mpar.release();
        mout.release();
    }
};

// n windows, window w in x + x_stride w; everything is checked before anything is enqueued
static int fw_solve_batch(mml_ctx* ctx, const char* who, int n, mml_fullwindow* const* fws, const int* first_slot,
                          const double* T_bl, double* x, size_t x_stride, mml_solve_summary* summaries, int* evaluations,
                          double* records0) {
    int Wmax = 0, rounds = 0;
    const auto refuse = [&](int code, int w, const char* what) { return mml_refuse(ctx, code, "%s: window %d: %s", who, w, what); };
    {
        std::vector<std::pair<const mml_fullwindow*, int>> seen(n);
        for (int w = 0; w < n; ++w) {
            const mml_fullwindow* fw = fws[w];
            if (!fw) return refuse(MML_ERR_INVALID, w, "null handle");
            const int W = fw->W;
            if (!(W >= 1 && W <= MAXW && first_slot[w] >= 0 && first_slot[w] <= ctx->B - W))
                return refuse(MML_ERR_INVALID, w, "window does not fit the scan slots");
            if (!(fw->opts.max_num_iterations >= 0 && fw->opts.max_num_iterations <= FW_MAX_ROUNDS - 1))
                return refuse(MML_ERR_INVALID, w, "max_num_iterations out of range");
            for (int f = 1; f < W; ++f)
                if (fw->have_imu[f] && !fw->U_ok[f]) return refuse(MML_ERR_STATE, w, "pre-integration covariance is not positive definite");
            seen[w] = {fw, w};
            Wmax = std::max(Wmax, W);
            rounds = std::max(rounds, fw->opts.max_num_iterations + 1);
        }
        std::sort(seen.begin(), seen.end());
        for (int i = 1; i < n; ++i)
            if (seen[i].first == seen[i - 1].first) return refuse(MML_ERR_INVALID, seen[i].second, "the same handle appears twice in the batch");
    }
    MML_HIP(hipSetDevice(ctx->device));
    MmlFwDev* d = mml_side<MmlFwDev>(ctx, MML_SIDE_FULLWINDOW);
    if (d->par.reserve(ctx, n) || d->state.reserve(ctx, n) || d->out.reserve(ctx, n) || d->alive.reserve(ctx, FW_MAX_ROUNDS) ||
        d->rec0.reserve(ctx, 32 * (size_t)n))
        return MML_ERR_HIP;
    // the per-window parameter blocks, staged in pinned memory; only what the kernels read is written (the flags of the
    // header gate every optional part)
    for (int w = 0; w < n; ++w) {
        const mml_fullwindow* fw = fws[w];
        const int W = fw->W;
        FwDevParams& p = d->par.h[w];
        memset(&p, 0, offsetof(FwDevParams, x));
        p.W = W;
        p.max_iters = fw->opts.max_num_iterations;
        p.fixed = fw->opts.fixed_iterations;
        p.first = first_slot[w];
        p.huber = fw->opts.huber_delta;
        p.w_tan = fw->opts.plan_weight_tan;
        memcpy(p.gravity, fw->gravity, sizeof(p.gravity));
        memcpy(p.Tbl, T_bl, sizeof(p.Tbl));
        memcpy(p.x, x + x_stride * w, sizeof(double) * 15 * W);
        p.has_prior = fw->prior.valid ? 1 : 0;
        if (fw->prior.valid) {
            p.prior = fw->prior.p;
            for (int a = 0; a < 15; ++a)
                for (int b = 0; b < 15; ++b) {
                    double h = 0;
                    for (int i = 0; i < 15; ++i) h += p.prior.J[i * 15 + a] * p.prior.J[i * 15 + b];
                    p.PP[a * 15 + b] = h;
                }
        }
        for (int f = 1; f < W; ++f) {
            if (!fw->have_imu[f]) continue;
            p.have_imu[f] = 1;
            p.imu[f] = fw->imu[f];
            memcpy(p.U[f], &fw->U[225 * (size_t)f], sizeof(p.U[f]));
        }
    }
    hipStream_t s = MML_STREAM(ctx);
    if (records0)  // (the records carry the used-factor counts of the association's statistics)
        for (int w = 0; w < n; ++w) {
            const int rs = mml_ensure_assoc_stats(ctx, first_slot[w], 1);
            if (rs != MML_OK) return rs;
        }
    MmlStageScope t(ctx, "fullwindow");
    MML_HIP(hipMemcpyAsync(d->par.d, d->par.h, sizeof(FwDevParams) * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_fw_init, dim3(1, n), dim3(128), 0, s, d->par.d, d->state.d, d->alive.d, rounds);
    FwKernelArgs a;
    a.P = d->par.d;
    a.G = d->state.d;
    a.out = d->out.d;
    a.alive = d->alive.d;
    a.ft_n = ctx->ft_n;
    a.lf = ctx->lf;
    a.pf = ctx->pf;
    a.B = ctx->B;
    a.MF = ctx->MF;
    // at most max_iterations + 1 evaluations: the first point and one candidate per iteration (an invalid step consumes
    // an iteration without an evaluation); the batch runs to its largest count.  Enqueued in chunks of four; the last
    // round of a chunk counts the windows that are still going and that count comes back (one 4-byte copy for the whole
    // batch), so that a batch that converged early does not pay for the launches of the remaining no-op rounds.
    for (int r = 0; r < rounds; ++r) {
        a.round = r;
        a.poll = (r & 3) == 3 && r + 1 < rounds;
        hipLaunchKernelGGL(k_fw_eval, dim3(2 * Wmax, n), dim3(SOLVE_THREADS), 0, s, a);
        hipLaunchKernelGGL(k_fw_step, dim3(1, n), dim3(FW_THREADS), 0, s, a);
        if (a.poll) {
            MML_HIP(hipGetLastError());
            MML_HIP(hipMemcpyAsync(&d->out.h->pad_, d->alive.d + r, sizeof(int), hipMemcpyDeviceToHost, s));
            MML_HIP(hipStreamSynchronize(s));
            if (!d->out.h->pad_) break;
        }
    }
    if (records0) hipLaunchKernelGGL(k_fw_record0, dim3(n), dim3(SOLVE_THREADS), 0, s, a, ctx->assoc_stats, d->rec0.d);
    MML_HIP(hipGetLastError());
    MML_HIP(hipMemcpyAsync(d->out.h, d->out.d, sizeof(FwDevOut) * n, hipMemcpyDeviceToHost, s));
    if (records0) MML_HIP(hipMemcpyAsync(d->rec0.h, d->rec0.d, sizeof(double) * 32 * n, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    if (records0) memcpy(records0, d->rec0.h, sizeof(double) * 32 * n);
    for (int w = 0; w < n; ++w) {
        mml_fullwindow* fw = fws[w];
        const int W = fw->W;
        const FwDevOut& o = d->out.h[w];
        double* xw = x + x_stride * w;
#ifdef MML_FW_TIMING
        {
            static const char* names[12] = {"assemble", "decide", "prep", "build", "factor_solve_rest", "dogleg", "xc", "fs_setup", "fs_chol", "fs_fwd", "fs_bwd", "chol_shader_clocks/100"};
            fprintf(stderr, "[fw step timing window=%d W=%d evals=%d iters=%d] us:", w, W, o.evaluations, o.iterations);
            for (int k = 0; k < 12; ++k) fprintf(stderr, " %s=%.1f", names[k], o.ticks[k] * 0.01);
            fprintf(stderr, "\n");
        }
#endif
        memcpy(xw, o.x, sizeof(double) * 15 * W);
        // the handle reports this solve through mml_fullwindow_summary, and marginalizes at the returned x
        fw->iter = o.iterations;
        fw->successful = o.successful;
        fw->termination = o.termination;
        fw->initial_cost = o.initial_cost;
        fw->cur.cost = o.final_cost;
        fw->started = fw->done = 1;
        fw->x.assign(xw, xw + 15 * W);
        if (summaries) {
            summaries[w].iterations = o.iterations;
            summaries[w].successful = o.successful;
            summaries[w].initial_cost = o.initial_cost;
            summaries[w].final_cost = o.final_cost;
            summaries[w].termination = o.termination;
        }
        if (evaluations) evaluations[w] = o.evaluations;
    }
    return MML_OK;
}

extern "C" int mml_fullwindow_solve(mml_ctx* ctx, mml_fullwindow* fw, int first_slot, const double* T_bl, double* x,
                                    mml_solve_summary* summary, int* evaluations) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(fw && T_bl && x, MML_ERR_INVALID, "mml_fullwindow_solve: null argument");
    return fw_solve_batch(ctx, "mml_fullwindow_solve", 1, &fw, &first_slot, T_bl, x, 0, summary, evaluations, nullptr);
}

extern "C" int mml_fullwindow_solve_batch(mml_ctx* ctx, int n, mml_fullwindow* const* fws, const int* first_slot,
                                          const double* T_bl, double* x, mml_solve_summary* summaries, int* evaluations,
                                          double* records0) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n >= 1 && n <= MML_FW_BATCH_MAX, MML_ERR_INVALID, "mml_fullwindow_solve_batch: n outside 1 .. MML_FW_BATCH_MAX");
    MML_REQUIRE(fws && first_slot && T_bl && x, MML_ERR_INVALID, "mml_fullwindow_solve_batch: null argument");
    return fw_solve_batch(ctx, "mml_fullwindow_solve_batch", n, fws, first_slot, T_bl, x, MML_FW_X_STRIDE, summaries, evaluations,
                          records0);
}

extern "C" int mml_fullwindow_marginalize_batch(mml_ctx* ctx, int n, mml_fullwindow* const* fws, const int* first_slot,
                                                const double* T_bl, const double* x, mml_prior* priors) {
    if (n < 1 || !fws || !first_slot || !T_bl || !x || !priors)
        return mml_refuse(ctx, MML_ERR_INVALID, "mml_fullwindow_marginalize_batch: n < 1 or a null argument");
    // (the argument checks come before anything needs a context; without one the refusal carries no message)
    const auto refuse = [&](int code, int w, const char* what) {
        return mml_refuse(ctx, code, "mml_fullwindow_marginalize_batch: window %d: %s", w, what);
    };
    if (n > MML_FW_BATCH_MAX) return refuse(MML_ERR_INVALID, MML_FW_BATCH_MAX, "the batch holds more than MML_FW_BATCH_MAX windows");
    for (int w = 0; w < n; ++w) {
        const mml_fullwindow* fw = fws[w];
        if (!fw) return refuse(MML_ERR_INVALID, w, "null handle");
        if (fw->W < 2) return refuse(MML_ERR_INVALID, w, "a window of one frame has nothing to marginalize");
        if (!fw->have_imu[1]) return refuse(MML_ERR_INVALID, w, "no IMU factor between frames 0 and 1");
        if (!(ctx && first_slot[w] >= 0 && first_slot[w] < ctx->B)) return refuse(MML_ERR_INVALID, w, "slot out of range");
        if (!fw->U_ok[1]) return refuse(MML_ERR_STATE, w, "pre-integration covariance is not positive definite");
    }
    MML_HIP(hipSetDevice(ctx->device));
    MmlFwDev* d = mml_side<MmlFwDev>(ctx, MML_SIDE_FULLWINDOW);
    if (d->mpar.reserve(ctx, n) || d->mout.reserve(ctx, n)) return MML_ERR_HIP;
    for (int w = 0; w < n; ++w) {  // only what the kernel reads is written (has_prior gates the prior)
        const mml_fullwindow* fw = fws[w];
        FwMargParams& p = d->mpar.h[w];
        p.first = first_slot[w];
        p.has_prior = fw->prior.valid ? 1 : 0;
        p.w_tan = fw->opts.plan_weight_tan;
        p.huber = 0.0;
        memcpy(p.gravity, fw->gravity, sizeof(p.gravity));
        memcpy(p.Tbl, T_bl, sizeof(p.Tbl));
        memcpy(p.x, x + (size_t)MML_FW_X_STRIDE * w, sizeof(p.x));
        if (fw->prior.valid) p.prior = fw->prior.p;
        p.imu = fw->imu[1];
        memcpy(p.U, &fw->U[225], sizeof(p.U));
    }
    hipStream_t s = MML_STREAM(ctx);
    MmlStageScope t(ctx, "fullwindow_marginalize");
    MML_HIP(hipMemcpyAsync(d->mpar.d, d->mpar.h, sizeof(FwMargParams) * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_fw_marginalize, dim3(n), dim3(SOLVE_THREADS), 0, s, d->mpar.d, d->mout.d, ctx->ft_n, ctx->lf, ctx->pf, ctx->B,
                       ctx->MF);
    MML_HIP(hipGetLastError());
    MML_HIP(hipMemcpyAsync(d->mout.h, d->mout.d, sizeof(mml_prior) * n, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    memcpy(priors, d->mout.h, sizeof(mml_prior) * n);
    return MML_OK;
}

extern "C" int mml_marginalize_dense(mml_ctx* ctx, long n, const double* A, const double* b, double* J, double* r0) {
    if (n < 0 || n > (long)1 << 20 || !A || !b || !J || !r0) return MML_ERR_INVALID;
    if (n == 0) return MML_OK;
    if (!ctx) {  // the host build of the routine, what mml_fullwindow_marginalize runs
        MargWork work;
        for (long w = 0; w < n; ++w) marg_dense(A + 900 * w, b + 30 * w, J + 225 * w, r0 + 15 * w, work);
        return MML_OK;
    }
    int rc = mml_sync_all(ctx);
    if (rc != MML_OK) return rc;
    MmlTemp<double> tmp;  // A | b | J | r0
    const size_t nA = 900 * (size_t)n, nb = 30 * (size_t)n, nJ = 225 * (size_t)n, nr = 15 * (size_t)n;
    bool ok = tmp.alloc(nA + nb + nJ + nr) == hipSuccess;
    double* d_buf = tmp.d;
    ok = ok && hipMemcpy(d_buf, A, sizeof(double) * nA, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(d_buf + nA, b, sizeof(double) * nb, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_marg_dense, dim3((unsigned)n), dim3(64), 0, MML_STREAM(ctx), (const double*)d_buf, (const double*)(d_buf + nA),
                           d_buf + nA + nb, d_buf + nA + nb + nJ);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(MML_STREAM(ctx)) == hipSuccess;
    }
    ok = ok && hipMemcpy(J, d_buf + nA + nb, sizeof(double) * nJ, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(r0, d_buf + nA + nb + nJ, sizeof(double) * nr, hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? MML_OK : MML_ERR_HIP;
}

extern "C" int mml_debug_fw_replay(mml_ctx* ctx, int variant, int n, const int* hdr, const double* x0, const long long* offsets,
                                   const double* rounds, long long rounds_len, double* xc, double* digest, int* digest_i) {
    if (variant < 0 || variant > 1 || n < 0 || n > MML_FW_REPLAY_SCRIPTS_MAX || !hdr || !x0 || !offsets || !rounds || !xc || !digest ||
        !digest_i || rounds_len < 0 || rounds_len > (64ll << 20) / (long long)sizeof(double) || (variant != 0 && !ctx))
        return MML_ERR_INVALID;
    std::vector<long long> row((size_t)n + 1, 0);
    for (int s = 0; s < n; ++s) {
        const int W = hdr[4 * s], fixed = hdr[4 * s + 1], max_iters = hdr[4 * s + 2], R = hdr[4 * s + 3];
        if (W < 1 || W > MAXW || (fixed != 0 && fixed != 1) || max_iters < 0 || max_iters > FW_MAX_ROUNDS - 1 || R < 1 ||
            R > MML_FW_REPLAY_ROUNDS_MAX)
            return MML_ERR_INVALID;
        const long long len = (long long)R * (46ll * 15 * W + 1);
        if (offsets[s] < 0 || offsets[s] > rounds_len - len) return MML_ERR_INVALID;
        row[s + 1] = row[s] + R;
    }
    if (n == 0) return MML_OK;
    const size_t no = (size_t)row[n], nxc = no * FW_N, nd = no * MML_FW_DIGEST_DOUBLES, ni = no * MML_TR_DIGEST_INTS;
    for (size_t i = 0; i < nxc; ++i) xc[i] = 0.0;
    for (size_t i = 0; i < nd; ++i) digest[i] = 0.0;
    for (size_t i = 0; i < ni; ++i) digest_i[i] = 0;
    MmlFwReplay P;
    P.n = n;
    if (variant == 0) {
        P.hdr = hdr;
        P.x0 = x0;
        P.off = offsets;
        P.row = row.data();
        P.rounds = rounds;
        P.xc = xc;
        P.dig = digest;
        P.digi = digest_i;
        for (int s = 0; s < n; ++s) mml_fw_replay_host(P, s);
        return MML_OK;
    }
    int rc = mml_sync_all(ctx);
    if (rc != MML_OK) return rc;
    MmlTemp<double> dbuf;     // x0 | rounds | xc | digest | the band slots
    MmlTemp<int> ibuf;        // hdr | digest_i
    MmlTemp<long long> lbuf;  // offsets | rows
    const size_t nx = (size_t)n * FW_N, nr = (size_t)rounds_len, nh = (size_t)n * 2 * FW_N * FW_BW;
    bool ok = dbuf.alloc(nx + nr + nxc + nd + nh) == hipSuccess && ibuf.alloc(4 * (size_t)n + ni) == hipSuccess &&
              lbuf.alloc(2 * (size_t)n) == hipSuccess;
    ok = ok && hipMemcpy(dbuf.d, x0, sizeof(double) * nx, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && (nr == 0 || hipMemcpy(dbuf.d + nx, rounds, sizeof(double) * nr, hipMemcpyHostToDevice) == hipSuccess);
    ok = ok && hipMemset(dbuf.d + nx + nr, 0, sizeof(double) * (nxc + nd + nh)) == hipSuccess;
    ok = ok && hipMemcpy(ibuf.d, hdr, sizeof(int) * 4 * (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemset(ibuf.d + 4 * (size_t)n, 0, sizeof(int) * ni) == hipSuccess;
    ok = ok && hipMemcpy(lbuf.d, offsets, sizeof(long long) * (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(lbuf.d + n, row.data(), sizeof(long long) * (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        P.hdr = ibuf.d;
        P.x0 = dbuf.d;
        P.off = lbuf.d;
        P.row = lbuf.d + n;
        P.rounds = dbuf.d + nx;
        P.xc = dbuf.d + nx + nr;
        P.dig = dbuf.d + nx + nr + nxc;
        P.digi = ibuf.d + 4 * (size_t)n;
        hipStream_t st = MML_STREAM(ctx);
        hipLaunchKernelGGL(k_fw_replay, dim3((unsigned)n), dim3(FW_THREADS), 0, st, P, dbuf.d + nx + nr + nxc + nd);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    }
    ok = ok && hipMemcpy(xc, P.xc, sizeof(double) * nxc, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(digest, P.dig, sizeof(double) * nd, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(digest_i, P.digi, sizeof(int) * ni, hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? MML_OK : MML_ERR_HIP;
}
