// gicp.hip -- SURVEY.md 8(f) rank 4: the per-frame GICP extrinsic refresh of the feature node on the device.
// Replaces icp_ext_matching (mm-loam/src/unionFeatureExtract.cpp:74-123, called at :302-312 with the Livox surf cloud as source
// and the Velodyne surf cloud as target): pcl::GeneralizedIterativeClosestPoint with setMaximumIterations(10),
// setTransformationEpsilon(1e-6) and PCL's defaults otherwise (20 correspondences per covariance, gicp_epsilon 1e-3,
// rotation_epsilon 2e-3, 20 inner BFGS iterations, no correspondence distance limit, identity guess).  PCL is not in the
// reference tree; this follows the published algorithm of PCL 1.8.1 (gicp.hpp; bfgs.h = GSL's vector_bfgs2 with
// Fletcher's line search).
//
// ONE set of kernels serves the single calls (mml_gicp_align, mml_gicp_refresh) and the batch calls (mml_gicp_align_batch,
// mml_gicp_refresh_batch): a call is n >= 1 independent alignments described by a table of GicpProb records, the problem index is
// blockIdx.y (blockIdx.x of k_gicp_bfgs), and the single calls are the n = 1 case.  A problem's arithmetic does not depend on
// what else is in the call, so a batch result equals the single call's bit for bit.
//
// What runs where (everything on the ctx stream, one read-back of 96 bytes per problem at the end):
//   k_gicp_cov   one lane per point: exact 20-NN in its own cloud by brute force over LDS tiles (the clouds are a few
//                hundred to a few thousand surf points -- the search grid of the association would cost more to build
//                than the N^2 distance tests), top-20 list as sorted 64-bit (distance, index) keys in registers, second
//                moments in neighbour order, symmetric eigen-solver, covariance = sum of v_k u_k u_k^T as PCL forms it (v = 1, 1, 1e-3)
//   k_gicp_corr  one lane per source point: transform with the current estimate, exact 1-NN in the target, Mahalanobis
//                matrix (R C1 R^T + C2)^-1
//   k_gicp_bfgs  ONE workgroup per problem: the whole inner BFGS minimisation of f(x) = 1/m sum res^T M res over x = (t, roll, pitch, yaw).
//                Every thread runs the (scalar) BFGS / line-search control flow on identical values; an objective
//                evaluation is a strided pass over the correspondences + a block reduction of 13 doubles, broadcast
//                back to all threads.  The kernel then forms the new 4 x 4 float transformation, the convergence measure
//                of the outer loop and the iteration count, so the host enqueues up to 10 (corr, bfgs) rounds blindly: a
//                converged or failed state turns the remaining rounds into no-ops.
//
// The three settings the reference's two call sites differ in travel with the call (GicpRun): the feature node's
// {10 iterations, transformation epsilon 1e-6, no correspondence gate} behind the entry points above, the caller's own behind
// mml_gicp_align_opts (the aligner's start-up calibration, calibrate.hip, uses {500, 1e-3, 2 m}).  The gate is PCL 1.8.1's
// computeTransformation: a source point whose 1-NN squared distance is not below the gate squared gets no correspondence
// (corr = -1); the objective skips it -- no term, and it does not count in the 1/m -- while every other point keeps its place i
// in the passes.  More than 10 iterations run as chunks of 10 rounds with one read-back of the states per chunk, until every
// problem has converged or failed: ceil(iterations run / 10) host synchronisations for the alignment, one with the feature node's settings.
#include <math.h>
#include <string.h>

#include "mml_internal.h"
#include "raw_gather_dev.h"

namespace {

#include "eig3_dev.h"

constexpr int GK = 20;            // k_correspondences_
constexpr int TILE = 1024;        // points per LDS tile of the brute-force searches
constexpr int BF_THREADS = 256;
constexpr double GICP_EPS = 1e-3, ROT_EPS = 2e-3;
constexpr int ROUNDS_PER_CHUNK = 10;  // (corr, bfgs) rounds enqueued between two read-backs of the states

// the settings of a call, as the kernels take them
struct GicpRun {
    int max_it;            // setMaximumIterations
    double inv_trans_eps;  // 1 / setTransformationEpsilon
    double gate2;          // setMaxCorrespondenceDistance squared; <= 0: no gate
};
constexpr GicpRun FEATURE_NODE_RUN = {10, 1.0 / 1e-6, 0.0};  // icp_ext_matching

struct GicpState {  // device-resident state of the outer loop, one per problem
    float T[16];    // transformation_ (row-major)
    int converged, failed, nr, evals;
    double fobj, delta;
};

// One alignment of a call: where its clouds and its per-point arrays sit in the call's block.  The clouds of all problems are
// packed into one float4 array; a point's covariance has the point's index, a source point's Mahalanobis matrix and
// correspondence the index moff + i.  n_src = n_tgt = 0: nothing to align (a skipped slot, a cloud of fewer than GK points) --
// every kernel leaves such a problem alone.
struct GicpProb {
    int src, tgt;      // first point of the source / target cloud
    int n_src, n_tgt;
    int moff;          // first entry of the source cloud in maha[] / corr[]
    int _pad;
};

__device__ __forceinline__ unsigned long long dkey(float d, int id) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)id;
}

// grid (blocks of the call's largest cloud, problems, 2): z = 0 the target clouds, 1 the source clouds.  A block wholly past its
// cloud's size leaves before the first barrier.  IDS (the test hook mml_debug_gicp only): the neighbour list of every point goes to
// nn_ids, GK ids per point in the list's order; the product's instantiation <false> never reads the pointer.
template <bool IDS>
__global__ __launch_bounds__(256) void k_gicp_cov(const GicpProb* __restrict__ tab, const float4* __restrict__ pts_all,
                                                  double* __restrict__ cov_all, int* __restrict__ nn_ids) {
    __shared__ float4 tile[TILE];
    const GicpProb P = tab[blockIdx.y];
    const int n = blockIdx.z ? P.n_src : P.n_tgt, first = blockIdx.z ? P.src : P.tgt;
    if ((int)(blockIdx.x * blockDim.x) >= n) return;
    const float4* __restrict__ pts = pts_all + first;
    double* __restrict__ cov = cov_all + 9 * (size_t)first;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float4 q = pts[i < n ? i : n - 1];
    unsigned long long k[GK];
#pragma unroll
    for (int j = 0; j < GK; ++j) k[j] = ~0ull;
    for (int base = 0; base < n; base += TILE) {
        const int cnt = min(TILE, n - base);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += blockDim.x) tile[t] = pts[base + t];
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const float4 p = tile[t];
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const float d = (dx * dx + dy * dy) + dz * dz;
            const unsigned long long key = dkey(d, base + t);
            if (key < k[GK - 1]) {
                k[GK - 1] = key;
#pragma unroll
                for (int j = GK - 1; j > 0; --j) {
                    const unsigned long long lo = k[j - 1] < k[j] ? k[j - 1] : k[j], hi = k[j - 1] < k[j] ? k[j] : k[j - 1];
                    k[j - 1] = lo;
                    k[j] = hi;
                }
            }
        }
    }
    if (i >= n) return;
    if (IDS) {
#pragma unroll
        for (int j = 0; j < GK; ++j) nn_ids[GK * (size_t)(first + i) + j] = (int)(unsigned)k[j];
    }
    // computeCovariances: sums in neighbour order, float products accumulated in double
    double mean[3] = {0, 0, 0}, c00 = 0, c10 = 0, c11 = 0, c20 = 0, c21 = 0, c22 = 0;
#pragma unroll
    for (int j = 0; j < GK; ++j) {
        const float4 p = pts[(unsigned)k[j]];
        mean[0] += p.x;
        mean[1] += p.y;
        mean[2] += p.z;
        c00 += p.x * p.x;
        c10 += p.y * p.x;
        c11 += p.y * p.y;
        c20 += p.z * p.x;
        c21 += p.z * p.y;
        c22 += p.z * p.z;
    }
    const double kk = static_cast<double>(GK);
    mean[0] /= kk;
    mean[1] /= kk;
    mean[2] /= kk;
    c00 = c00 / kk - mean[0] * mean[0];
    c10 = c10 / kk - mean[1] * mean[0];
    c11 = c11 / kk - mean[1] * mean[1];
    c20 = c20 / kk - mean[2] * mean[0];
    c21 = c21 / kk - mean[2] * mean[1];
    c22 = c22 / kk - mean[2] * mean[2];
    double ev[3], u2[3], u0[3], u1[3];
    eig3_sym(c00, c10, c11, c20, c21, c22, ev, u2, u0, u1);
    // PCL (gicp.hpp computeCovariances): cov = sum_k v_k col_k col_k^T over the columns of U in the SVD's order -- singular values
    // descending --, v = 1, 1, gicp_epsilon; each term is (v col[r]) col[s], added to the matrix one k after the other
    double* o = cov + 9 * (size_t)i;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            double a = 0.0;
            a += (1.0 * u2[r]) * u2[s];
            a += (1.0 * u1[r]) * u1[s];
            a += (GICP_EPS * u0[r]) * u0[s];
            o[3 * r + s] = a;
        }
}

__device__ __forceinline__ void tf_pt(const float* T, float x, float y, float z, float* o) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3];
}

// grid (blocks of the call's largest source cloud, problems)
__global__ __launch_bounds__(256) void k_gicp_corr(const GicpProb* __restrict__ tab, const float4* __restrict__ pts_all,
                                                   const double* __restrict__ cov_all, const GicpState* st_all, int* __restrict__ corr_all,
                                                   double* __restrict__ maha_all, double gate2) {
    __shared__ float4 tile[TILE];
    const GicpProb P = tab[blockIdx.y];
    const int ns = P.n_src, nt = P.n_tgt;
    if ((int)(blockIdx.x * blockDim.x) >= ns) return;
    const GicpState* st = st_all + blockIdx.y;
    if (st->converged || st->failed) return;
    const float4* __restrict__ src = pts_all + P.src;
    const float4* __restrict__ tgt = pts_all + P.tgt;
    const double* __restrict__ csrc = cov_all + 9 * (size_t)P.src;
    const double* __restrict__ ctgt = cov_all + 9 * (size_t)P.tgt;
    int* __restrict__ corr = corr_all + P.moff;
    double* __restrict__ maha = maha_all + 9 * (size_t)P.moff;
    float T[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) T[c] = st->T[c];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float4 p = src[i < ns ? i : ns - 1];
    float q[3];
    tf_pt(T, p.x, p.y, p.z, q);
    unsigned long long best = ~0ull;
    for (int base = 0; base < nt; base += TILE) {
        const int cnt = min(TILE, nt - base);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += blockDim.x) tile[t] = tgt[base + t];
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const float4 g = tile[t];
            const float dx = g.x - q[0], dy = g.y - q[1], dz = g.z - q[2];
            const float d = (dx * dx + dy * dy) + dz * dz;
            const unsigned long long key = dkey(d, base + t);
            best = key < best ? key : best;
        }
    }
    if (i >= ns) return;
    const int j = (int)(unsigned)best;
    // if (nn_dists[0] < dist_threshold) (gicp.hpp computeTransformation): the float the search produced against the double gate
    if (gate2 > 0.0 && !((double)__uint_as_float((unsigned)(best >> 32)) < gate2)) {
        corr[i] = -1;
        return;
    }
    corr[i] = j;
    double R[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)T[4 * r + c];
    const double* C1 = csrc + 9 * (size_t)i;
    const double* C2 = ctgt + 9 * (size_t)j;
    double RC[9], a[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) RC[3 * r + c] = (R[3 * r] * C1[c] + R[3 * r + 1] * C1[3 + c]) + R[3 * r + 2] * C1[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            a[3 * r + c] = ((RC[3 * r] * R[3 * c] + RC[3 * r + 1] * R[3 * c + 1]) + RC[3 * r + 2] * R[3 * c + 2]) + C2[3 * r + c];
    // 3 x 3 inverse by cofactors (Eigen's fixed-size inverse)
    const double k00 = a[4] * a[8] - a[5] * a[7], k01 = a[5] * a[6] - a[3] * a[8], k02 = a[3] * a[7] - a[4] * a[6];
    const double det = (a[0] * k00 + a[1] * k01) + a[2] * k02;
    const double id = 1.0 / det;
    double* M = maha + 9 * (size_t)i;
    M[0] = k00 * id;
    M[1] = (a[2] * a[7] - a[1] * a[8]) * id;
    M[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    M[3] = k01 * id;
    M[4] = (a[0] * a[8] - a[2] * a[6]) * id;
    M[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    M[6] = k02 * id;
    M[7] = (a[1] * a[6] - a[0] * a[7]) * id;
    M[8] = (a[0] * a[4] - a[1] * a[3]) * id;
}

// ---- the inner BFGS, executed by every thread of one workgroup on identical values --------------------------------------
__device__ void apply_state(const double* x, float* T) {  // GeneralizedIterativeClosestPoint::applyState on the identity
    // Eigen::AngleAxisf: cos / sin of the float angle, through the double functions (platform-independent rounding)
    const float cz = (float)cos((double)(float)x[5]), sz = (float)sin((double)(float)x[5]);
    const float cy = (float)cos((double)(float)x[4]), sy = (float)sin((double)(float)x[4]);
    const float cx = (float)cos((double)(float)x[3]), sx = (float)sin((double)(float)x[3]);
    const float Rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1}, Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy}, Rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx};
    float A[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[3 * r + c] = (Rz[3 * r] * Ry[c] + Rz[3 * r + 1] * Ry[3 + c]) + Rz[3 * r + 2] * Ry[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[4 * r + c] = (A[3 * r] * Rx[c] + A[3 * r + 1] * Rx[3 + c]) + A[3 * r + 2] * Rx[6 + c];
        T[4 * r + 3] = (float)x[r];
    }
    T[12] = T[13] = T[14] = 0.f;
    T[15] = 1.f;
}

// the state x = (t, roll, pitch, yaw) a 4 x 4 float transformation stands for (gicp.hpp computeTransformation's opening)
__device__ __forceinline__ void state_of(const float* T, double* x) {
    x[0] = (double)T[3];
    x[1] = (double)T[7];
    x[2] = (double)T[11];
    x[3] = atan2((double)T[9], (double)T[10]);
    x[4] = asin(-(double)T[8]);
    x[5] = atan2((double)T[4], (double)T[0]);
}

constexpr int EV_CH = 512;            // correspondences per LDS chunk of an objective evaluation
constexpr int EV_ROW = EV_CH + 1;     // row stride of the term table (odd number of 8-byte words: the 13 summing lanes hit 13 banks)
struct EvalCtx {
    const float4* src;
    const float4* tgt;
    const int* corr;
    const double* maha;
    int n;            // source points = positions of the strided pass
    int m;            // correspondences: n without a gate, else the points with corr >= 0
    double* s_terms;  // LDS: 13 rows x EV_ROW terms of the current chunk
    double* s_tot;    // LDS: the 13 totals
    int* s_keep;      // LDS: EV_CH flags "has a correspondence" of the current chunk; null without a gate
};

// OptimizationFunctorWithIndices::operator() / fdf: every thread returns the same f and (optionally) gradient.
// PCL adds the m terms of every sum one after the other; so does this: the terms of a chunk of correspondences are formed in
// parallel into an LDS table and ONE lane per sum adds them in correspondence order (the 13 sums on 13 lanes at once), so
// that f and the gradient equal the sequential loop's bit for bit -- the line search compares objective values that differ
// in their last bits near the flat minimum of a cross-sensor alignment, and a strided pass with a tree reduction decides
// some of those comparisons the other way (round 2: matrices equal to 5e-3 only).
// With a gate, a point without a correspondence forms no term and the summing lanes step over its place.
__device__ double gicp_eval(const EvalCtx& E, const double* x, double* g) {
    float T[16];
    apply_state(x, T);
    const int nsum = g ? 13 : 1;
    double run = 0;
    for (int c0 = 0; c0 < E.n; c0 += EV_CH) {
        const int cnt = min(EV_CH, E.n - c0);
        for (int j = threadIdx.x; j < cnt; j += BF_THREADS) {
            const int i = c0 + j;
            const int ci = E.corr[i];
            if (E.s_keep) {
                E.s_keep[j] = ci >= 0;
                if (ci < 0) continue;
            }
            const float4 ps = E.src[i], pt = E.tgt[ci];
            float pp[3];
            tf_pt(T, ps.x, ps.y, ps.z, pp);
            const double res[3] = {(double)(pp[0] - pt.x), (double)(pp[1] - pt.y), (double)(pp[2] - pt.z)};
            const double* M = E.maha + 9 * (size_t)i;
            double tmp[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) tmp[r] = (M[3 * r] * res[0] + M[3 * r + 1] * res[1]) + M[3 * r + 2] * res[2];
            E.s_terms[j] = (res[0] * tmp[0] + res[1] * tmp[1]) + res[2] * tmp[2];
            if (g) {
                const double p3[3] = {(double)ps.x, (double)ps.y, (double)ps.z};
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    E.s_terms[(1 + r) * EV_ROW + j] = tmp[r];
#pragma unroll
                    for (int c = 0; c < 3; ++c) E.s_terms[(4 + 3 * r + c) * EV_ROW + j] = p3[r] * tmp[c];
                }
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < nsum) {
            const double* row = E.s_terms + threadIdx.x * EV_ROW;
            if (E.s_keep) {
                for (int j = 0; j < cnt; ++j)
                    if (E.s_keep[j]) run += row[j];
            } else {
                for (int j = 0; j < cnt; ++j) run += row[j];
            }
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < nsum) E.s_tot[threadIdx.x] = run;
    __syncthreads();
    double tot[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) tot[k] = k < nsum ? E.s_tot[k] : 0.0;
    __syncthreads();
    const double m = (double)E.m;
    if (g) {
        double Rm[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) g[r] = tot[1 + r] * (2.0 / m);
#pragma unroll
        for (int k = 0; k < 9; ++k) Rm[k] = tot[4 + k] * (2.0 / m);
        // computeRDerivative
        const double phi = x[3], theta = x[4], psi = x[5];
        const double cphi = cos(phi), sphi = sin(phi), cth = cos(theta), sth = sin(theta), cpsi = cos(psi), spsi = sin(psi);
        const double dPhi[9] = {0, sphi * spsi + cphi * cpsi * sth, cphi * spsi - cpsi * sphi * sth,
                                0, -cpsi * sphi + cphi * spsi * sth, -cphi * cpsi - sphi * spsi * sth,
                                0, cphi * cth, -cth * sphi};
        const double dTh[9] = {-cpsi * sth, cpsi * cth * sphi, cphi * cpsi * cth,
                               -spsi * sth, cth * sphi * spsi, cphi * cth * spsi,
                               -cth, -sphi * sth, -cphi * sth};
        const double dPsi[9] = {-cth * spsi, -cphi * cpsi - sphi * spsi * sth, cpsi * sphi - cphi * spsi * sth,
                                cpsi * cth, -cphi * spsi + cpsi * sphi * sth, sphi * spsi + cphi * cpsi * sth,
                                0, 0, 0};
        double g3 = 0, g4 = 0, g5 = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                g3 += dPhi[3 * j + i] * Rm[3 * i + j];
                g4 += dTh[3 * j + i] * Rm[3 * i + j];
                g5 += dPsi[3 * j + i] * Rm[3 * i + j];
            }
        g[3] = g3;
        g[4] = g4;
        g[5] = g5;
    }
    return tot[0] / m;
}

__device__ __forceinline__ double cubic(double c0, double c1, double c2, double c3, double z) { return c0 + z * (c1 + z * (c2 + z * c3)); }
__device__ __forceinline__ void check_extremum(double c0, double c1, double c2, double c3, double z, double& zmin, double& fmin) {
    const double y = cubic(c0, c1, c2, c3, z);
    if (y < fmin) {
        zmin = z;
        fmin = y;
    }
}
__device__ int solve_quadratic(double a, double b, double c, double& x0, double& x1) {
    if (a == 0) {
        if (b == 0) return 0;
        x0 = -c / b;
        return 1;
    }
    const double disc = b * b - 4 * a * c;
    if (disc > 0) {
        if (b == 0) {
            const double r = sqrt(-c / a);
            x0 = -r;
            x1 = r;
        } else {
            const double sgnb = b > 0 ? 1 : -1;
            const double temp = -0.5 * (b + sgnb * sqrt(disc));
            const double r1 = temp / a, r2 = c / temp;
            x0 = r1 < r2 ? r1 : r2;
            x1 = r1 < r2 ? r2 : r1;
        }
        return 2;
    }
    if (disc == 0) {
        x0 = -0.5 * b / a;
        x1 = x0;
        return 2;
    }
    return 0;
}
__device__ double interpolate(double a, double fa, double fpa, double b, double fb, double fpb, double xmin, double xmax) {
    double ymin = (xmin - a) / (b - a), ymax = (xmax - a) / (b - a);
    if (ymin > ymax) {
        const double t = ymin;
        ymin = ymax;
        ymax = t;
    }
    const double f0 = fa, fp0 = fpa * (b - a), f1 = fb;
    double zmin, fmin;
    if (isfinite(fpb)) {  // cubic through both slopes
        const double fp1 = fpb * (b - a);
        const double eta = 3 * (f1 - f0) - 2 * fp0 - fp1, xi = fp0 + fp1 - 2 * (f1 - f0);
        zmin = ymin;
        fmin = cubic(f0, fp0, eta, xi, ymin);
        check_extremum(f0, fp0, eta, xi, ymax, zmin, fmin);
        double z0 = 0, z1 = 0;
        const int n = solve_quadratic(3 * xi, 2 * eta, fp0, z0, z1);
        if (n >= 1 && z0 > ymin && z0 < ymax) check_extremum(f0, fp0, eta, xi, z0, zmin, fmin);
        if (n == 2 && z1 > ymin && z1 < ymax) check_extremum(f0, fp0, eta, xi, z1, zmin, fmin);
    } else {  // quadratic
        const double fl = f0 + ymin * (fp0 + ymin * (f1 - f0 - fp0)), fh = f0 + ymax * (fp0 + ymax * (f1 - f0 - fp0));
        const double c = 2 * (f1 - f0 - fp0);
        zmin = ymin;
        fmin = fl;
        if (fh < fmin) {
            zmin = ymax;
            fmin = fh;
        }
        if (c > 0) {
            const double z = -fp0 / c;
            if (z > ymin && z < ymax) {
                const double f = f0 + z * (fp0 + z * (f1 - f0 - fp0));
                if (f < fmin) {
                    zmin = z;
                    fmin = f;
                }
            }
        }
    }
    return a + zmin * (b - a);
}

struct Bfgs {  // vector_bfgs2 state + the line wrapper with its caches (bfgs.h)
    double x0[6], g0[6], p[6];
    double step, g0norm, pnorm, delta_f, fp0;
    double f_alpha, df_alpha, x_alpha[6], g_alpha[6], f_key, df_key, x_key, g_key;
    double x[6], f, g[6];
    int evals;
};
__device__ __forceinline__ double nrm6(const double* v) {
    double s = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) s += v[i] * v[i];
    return sqrt(s);
}
__device__ __forceinline__ double dot6(const double* a, const double* b) {
    double s = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) s += a[i] * b[i];
    return s;
}
__device__ __forceinline__ void moveto(Bfgs& B, double alpha) {
    if (alpha == B.x_key) return;
#pragma unroll
    for (int i = 0; i < 6; ++i) B.x_alpha[i] = B.x0[i] + alpha * B.p[i];
    B.x_key = alpha;
}
__device__ double wf(Bfgs& B, const EvalCtx& E, double alpha) {
    if (alpha == B.f_key) return B.f_alpha;
    moveto(B, alpha);
    B.f_alpha = gicp_eval(E, B.x_alpha, nullptr);
    ++B.evals;
    B.f_key = alpha;
    return B.f_alpha;
}
__device__ double wdf(Bfgs& B, const EvalCtx& E, double alpha) {
    if (alpha == B.df_key) return B.df_alpha;
    moveto(B, alpha);
    if (alpha != B.g_key) {
        gicp_eval(E, B.x_alpha, B.g_alpha);
        ++B.evals;
        B.g_key = alpha;
    }
    B.df_alpha = dot6(B.g_alpha, B.p);
    B.df_key = alpha;
    return B.df_alpha;
}
__device__ void wfdf(Bfgs& B, const EvalCtx& E, double alpha, double& fo, double& dfo) {
    if (alpha == B.f_key && alpha == B.df_key) {
        fo = B.f_alpha;
        dfo = B.df_alpha;
        return;
    }
    if (alpha == B.f_key || alpha == B.df_key) {
        fo = wf(B, E, alpha);
        dfo = wdf(B, E, alpha);
        return;
    }
    moveto(B, alpha);
    B.f_alpha = gicp_eval(E, B.x_alpha, B.g_alpha);
    ++B.evals;
    B.f_key = alpha;
    B.g_key = alpha;
    B.df_alpha = dot6(B.g_alpha, B.p);
    B.df_key = alpha;
    fo = B.f_alpha;
    dfo = B.df_alpha;
}
__device__ void prepare_wrapper(Bfgs& B) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        B.x_alpha[i] = B.x0[i];
        B.g_alpha[i] = B.g0[i];
    }
    B.x_key = 0.0;
    B.f_alpha = B.f;
    B.f_key = 0.0;
    B.g_key = 0.0;
    B.df_alpha = dot6(B.g_alpha, B.p);
    B.df_key = 0.0;
}
// Fletcher's line search (linear_minimize.c): 0 success, 1 no progress
__device__ int line_search(Bfgs& B, const EvalCtx& E, double alpha1, double& alpha_new) {
    const double rho = 0.01, sigma = 0.01, tau1 = 9, tau2 = 0.05, tau3 = 0.5;
    double f0, fp0, falpha, falpha_prev, fpalpha = 0, fpalpha_prev, delta;
    double alpha = alpha1, alpha_prev = 0.0;
    double a = 0.0, b = alpha, fa, fb = 0.0, fpa, fpb = 0.0;
    int i = 0;
    wfdf(B, E, 0.0, f0, fp0);
    falpha_prev = f0;
    fpalpha_prev = fp0;
    fa = f0;
    fpa = fp0;
    while (i++ < 100) {
        falpha = wf(B, E, alpha);
        if (falpha > f0 + alpha * rho * fp0 || falpha >= falpha_prev) {
            a = alpha_prev;
            fa = falpha_prev;
            fpa = fpalpha_prev;
            b = alpha;
            fb = falpha;
            fpb = NAN;
            break;
        }
        fpalpha = wdf(B, E, alpha);
        if (fabs(fpalpha) <= -sigma * fp0) {
            alpha_new = alpha;
            return 0;
        }
        if (fpalpha >= 0) {
            a = alpha;
            fa = falpha;
            fpa = fpalpha;
            b = alpha_prev;
            fb = falpha_prev;
            fpb = fpalpha_prev;
            break;
        }
        delta = alpha - alpha_prev;
        const double alpha_next = interpolate(alpha_prev, falpha_prev, fpalpha_prev, alpha, falpha, fpalpha, alpha + delta, alpha + tau1 * delta);
        alpha_prev = alpha;
        falpha_prev = falpha;
        fpalpha_prev = fpalpha;
        alpha = alpha_next;
    }
    while (i++ < 100) {
        delta = b - a;
        alpha = interpolate(a, fa, fpa, b, fb, fpb, a + tau2 * delta, b - tau3 * delta);
        falpha = wf(B, E, alpha);
        if ((a - alpha) * fpa <= 2.220446049250313e-16) return 1;
        if (falpha > f0 + rho * alpha * fp0 || falpha >= fa) {
            b = alpha;
            fb = falpha;
            fpb = NAN;
        } else {
            fpalpha = wdf(B, E, alpha);
            if (fabs(fpalpha) <= -sigma * fp0) {
                alpha_new = alpha;
                return 0;
            }
            if (((b - a) >= 0 && fpalpha >= 0) || ((b - a) <= 0 && fpalpha <= 0)) {
                b = a;
                fb = fa;
                fpb = fpa;
            }
            a = alpha;
            fa = falpha;
            fpa = fpalpha;
        }
    }
    alpha_new = alpha;
    return 0;
}
__device__ int bfgs_iterate(Bfgs& B, const EvalCtx& E) {
    double alpha = 0.0, alpha1;
    const double f0 = B.f;
    if (B.pnorm == 0.0 || B.g0norm == 0.0 || B.fp0 == 0) return 1;
    if (B.delta_f < 0) {
        const double del = fmax(-B.delta_f, 10 * 2.220446049250313e-16 * fabs(f0));
        alpha1 = fmin(1.0, 2.0 * del / (-B.fp0));
    } else {
        alpha1 = fabs(B.step);
    }
    const int status = line_search(B, E, alpha1, alpha);
    if (status != 0) return status;
    double fn, dfn;
    wfdf(B, E, alpha, fn, dfn);
    double dx0[6], dg0[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        B.x[i] = B.x_alpha[i];
        B.g[i] = B.g_alpha[i];
        dx0[i] = B.x[i] - B.x0[i];
        dg0[i] = B.g[i] - B.g0[i];
    }
    B.f = fn;
    B.delta_f = B.f - f0;
    const double dxg = dot6(dx0, B.g), dgg = dot6(dg0, B.g), dxdg = dot6(dx0, dg0), dgnorm = nrm6(dg0);
    double A = 0, Bc = 0;
    if (dxdg != 0) {
        Bc = dxg / dxdg;
        A = -(1.0 + dgnorm * dgnorm / dxdg) * Bc + dgg / dxdg;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        B.p[i] = (B.g[i] - A * dx0[i]) - Bc * dg0[i];
        B.g0[i] = B.g[i];
        B.x0[i] = B.x[i];
    }
    B.g0norm = nrm6(B.g0);
    B.pnorm = nrm6(B.p);
    const double pg = dot6(B.p, B.g);
    const double dir = (pg >= 0.0) ? -1.0 : +1.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) B.p[i] *= dir / B.pnorm;
    B.pnorm = nrm6(B.p);
    B.fp0 = dot6(B.p, B.g0);
    prepare_wrapper(B);
    return 0;
}

// grid (problems): one workgroup per problem.  s_terms + s_tot are 13 x 513 + 13 doubles = 53,456 bytes of LDS, the gate's flags
// 2,052 more: a CU's 160 KiB (163,840 bytes) hold two such workgroups.  The scalar BFGS state costs about 200 VGPRs per lane, which
// allows two waves per SIMD, and a workgroup puts one wave on each of the four SIMDs: registers bound a CU to TWO workgroups as
// well -- 512 problems resident on the 256 CUs at once, the rest queue behind them.
__global__ __launch_bounds__(BF_THREADS) void k_gicp_bfgs(const GicpProb* __restrict__ tab, const float4* pts_all, const int* corr_all,
                                                         const double* maha_all, GicpState* st_all, GicpRun run) {
    __shared__ double s_terms[13 * EV_ROW];
    __shared__ double s_tot[13];
    __shared__ int s_keep[EV_CH];
    __shared__ int s_m;
    const GicpProb P = tab[blockIdx.x];
    const int n = P.n_src;
    if (n == 0) return;
    GicpState* st = st_all + blockIdx.x;
    if (st->converged || st->failed) return;
    const float4* src = pts_all + P.src;
    const float4* tgt = pts_all + P.tgt;
    const int* corr = corr_all + P.moff;
    const double* maha = maha_all + 9 * (size_t)P.moff;
    const bool gated = run.gate2 > 0.0;  // (workgroup-uniform)
    int m = n;
    if (gated) {  // the round's correspondence list: the points k_gicp_corr kept
        if (threadIdx.x == 0) s_m = 0;
        __syncthreads();
        int mine = 0;
        for (int i = threadIdx.x; i < n; i += BF_THREADS) mine += corr[i] >= 0;
        if (mine) atomicAdd(&s_m, mine);
        __syncthreads();
        m = s_m;
    }
    if (m < 4) {  // NotEnoughPointsException: the outer loop ends unconverged
        if (threadIdx.x == 0) st->failed = 1;
        return;
    }
    EvalCtx E{src, tgt, corr, maha, n, m, s_terms, s_tot, gated ? s_keep : nullptr};
    float T[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) T[c] = st->T[c];
    Bfgs B;
    double xin[6];
    state_of(T, xin);
    B.step = 1.0;
    B.delta_f = 0;
    B.evals = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) B.x[i] = xin[i];
    B.f = gicp_eval(E, B.x, B.g);
    ++B.evals;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        B.x0[i] = B.x[i];
        B.g0[i] = B.g[i];
    }
    B.g0norm = nrm6(B.g0);
#pragma unroll
    for (int i = 0; i < 6; ++i) B.p[i] = B.g[i] * (-1.0 / B.g0norm);
    B.pnorm = nrm6(B.p);
    B.fp0 = -B.g0norm;
    prepare_wrapper(B);
    int inner = 0, result = 0;
    do {
        ++inner;
        result = bfgs_iterate(B, E);
        if (result) break;
        result = nrm6(B.g) < 1e-2 ? 2 : 0;  // testGradient(gradient_tol)
    } while (result == 0 && inner < 20);
    float Tn[16];
    apply_state(B.x, Tn);
    double delta = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const double ratio = (k < 3 && l < 3) ? 1.0 / ROT_EPS : run.inv_trans_eps;
            const double cd = ratio * fabs((double)T[4 * k + l] - (double)Tn[4 * k + l]);
            delta = cd > delta ? cd : delta;
        }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 16; ++c) st->T[c] = Tn[c];
        st->nr += 1;
        st->evals += B.evals;
        st->fobj = B.f;
        st->delta = delta;
        if (st->nr >= run.max_it || delta < 1) st->converged = 1;
    }
}

__global__ void k_gicp_init(GicpState* st_all) {  // grid (problems)
    GicpState* st = st_all + blockIdx.x;
    if (threadIdx.x < 16) st->T[threadIdx.x] = (threadIdx.x % 5 == 0) ? 1.f : 0.f;
    if (threadIdx.x == 0) {
        st->converged = 0;
        st->failed = 0;
        st->nr = 0;
        st->evals = 0;
        st->fobj = 0;
        st->delta = 0;
    }
}

// The slots' surf clouds as the feature node builds them (unionFeatureExtract.cpp:1024-1031, :1242-1252): the points labelled 2 in
// the order of the sensor's RAW cloud, the Velodyne one cropped near + far (:1287-1293), the Livox one near only (:925) --
// its labelled points beyond far_th carry bit 7 in their label byte.  One workgroup per (sensor, slot) walks the raw line ids in
// order and rebuilds every point's bucketed position, which is where its label and its coordinates live (raw_gather_dev.h).
// grid (2, slots), run twice: the count pass (tab == nullptr) leaves counts[2 i + sensor] for the host to lay the call's clouds
// out -- 0, 0 for a slot the refresh skips (livox_corner_num <= 100) --, the write pass puts the clouds of the problems that align
// at their offsets in pts.
struct GatherArgs {
    const uint8_t* raw_line;
    const int *n_in, *seg_flat, *seg_flat_n, *fu_info;
    const uint8_t* label;
    const float4* ln_pts;
    int first, NT, NV, blk_points;
};
__global__ __launch_bounds__(RG_THREADS) void k_gicp_gather_raw(GatherArgs A, const GicpProb* tab, float4* pts, int* counts) {
    const int sensor = blockIdx.x, slot = A.first + blockIdx.y;
    float4* out = nullptr;
    if (tab) {
        const GicpProb P = tab[blockIdx.y];
        if (P.n_src == 0) return;
        out = pts + (sensor == 0 ? P.tgt : P.src);
    } else if (!(A.fu_info[8 * (size_t)slot + 4] > 100)) {  // union_msg.livox_corner_num > 100 (unionFeatureExtract.cpp:302)
        if (threadIdx.x == 0) counts[2 * blockIdx.y + sensor] = 0;
        return;
    }
    const size_t o = (size_t)slot * A.NT;
    const uint8_t* label = A.label + o;
    const float4* ln_pts = A.ln_pts + o;
    const RawGatherSrc S{A.raw_line + o + (sensor == 0 ? 0 : A.NV), A.seg_flat + ((size_t)slot * 2 + sensor) * MML_SEG_FLAT,
                         A.n_in[2 * (size_t)slot + sensor], A.seg_flat_n[(size_t)slot * 4 + 2 * sensor + 1], A.blk_points, MML_SEG_FLAT, A.NT};
    const unsigned lim = sensor == 0 ? 0x80u : 0x100u;
    int n_out[2];
    raw_gather_walk(
        S,
        [&](int p) {
            const unsigned l = label[p];
            return ((l & 3u) == 2u && l < lim) ? 0 : -1;
        },
        [&](int, int at, int, int p, int) {
            if (out) out[at] = ln_pts[p];
        },
        n_out);
    if (!tab && threadIdx.x == 0) counts[2 * blockIdx.y + sensor] = n_out[0];
}

// pcl::transformPointCloud, float (PCL 1.8.1), on the Livox regions of the slots first .. : grid (blocks of the largest region,
// slots), slot i's matrix is T + 16 i and its point count n[i] (0: not transformed)
__global__ void k_gicp_apply(float4* ln_pts, int first, int NT, int NV, const int* n, const float* T_all) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n[blockIdx.y]) return;
    float4* pts = ln_pts + (size_t)(first + blockIdx.y) * NT + NV;
    const float* T = T_all + 16 * (size_t)blockIdx.y;
    float4 p = pts[i];
    const float x = T[0] * p.x + T[1] * p.y + T[2] * p.z + T[3];
    const float y = T[4] * p.x + T[5] * p.y + T[6] * p.z + T[7];
    const float z = T[8] * p.x + T[9] * p.y + T[10] * p.z + T[11];
    p.x = x;
    p.y = y;
    p.z = z;
    pts[i] = p;
}

// io block (device + pinned twin) of a call of n problems: what crosses the bus.  `pts`: the packed clouds of mml_gicp_align*,
// which come from the host (the refresh gathers its clouds on the device, into the big block)
struct GicpIo {
    MmlCarve<16> c;
    MmlField<GicpProb> tab;
    MmlField<GicpState> st;
    MmlField<int> cnt;
    MmlField<float> mat;
    MmlField<int> napp, fi, cb, fl;
    MmlField<float4> pts;
    size_t bytes;
    GicpIo(size_t n, size_t n_pts)
        : tab(c.take<GicpProb>(n)), st(c.take<GicpState>(n)), cnt(c.take<int>(2 * n)), mat(c.take<float>(16 * n)), napp(c.take<int>(n)),
          fi(c.take<int>(8 * n)), cb(c.take<int>(2 * n)), fl(c.take<int>(2 * n)), pts(c.take<float4>(n_pts)), bytes(c.bytes()) {}
};
// big block (device only): 72 bytes of covariance per point, 72 + 4 bytes per source point, and the refresh's 16 bytes per point
struct GicpBig {
    MmlCarve<16> c;
    MmlField<float4> pts;
    MmlField<double> cov, maha;
    MmlField<int> corr;
    size_t bytes;
    GicpBig(size_t n_pts, size_t n_srcs, bool with_pts)
        : pts(c.take<float4>(with_pts ? n_pts : 0)), cov(c.take<double>(9 * n_pts)), maha(c.take<double>(9 * n_srcs)), corr(c.take<int>(n_srcs)),
          bytes(c.bytes()) {}
};

}  // namespace

// Grow-only scratch of the alignments, owned by the context: nothing is allocated or freed per call once the largest call has
// been seen.  Every entry point drains the stream before it returns, so reserve() never replaces a buffer in use.
struct MmlGicpDev {
    MmlStaging<char> io;
    MmlStaging<char, false> big;
    ~MmlGicpDev() {
        io.release();
        big.release();
    }
};

namespace {

// Lays problem `P` of ns source and nt target points out behind the n_pts points and n_srcs source points already placed.
// PCL: "number of points smaller than k_correspondences_" -> no alignment: such a problem gets no room and n_src = n_tgt = 0.
void place_problem(GicpProb& P, int ns, int nt, size_t& n_pts, size_t& n_srcs) {
    memset(&P, 0, sizeof(P));
    if (ns < GK || nt < GK) return;
    P.src = (int)n_pts;
    P.tgt = (int)(n_pts + ns);
    P.n_src = ns;
    P.n_tgt = nt;
    P.moff = (int)n_srcs;
    n_pts += (size_t)ns + nt;
    n_srcs += ns;
}

// The launch sequence of a call: the n alignments of d_tab on the clouds in pts, states read back into h_st: one host
// synchronisation per chunk of ROUNDS_PER_CHUNK rounds, so one up to 10 iterations.  max_src / max_tgt: the largest clouds among
// the problems that align.
int gicp_core(mml_ctx* ctx, const GicpRun& run, int n, int max_src, int max_tgt, const GicpProb* d_tab, const float4* pts, double* cov,
              double* maha, int* corr, GicpState* d_st, GicpState* h_st) {
    hipStream_t s = MML_STREAM(ctx);
    MmlStageScope t(ctx, "gicp");
    const int max_c = max_src > max_tgt ? max_src : max_tgt;
    hipLaunchKernelGGL(k_gicp_init, dim3(n), dim3(64), 0, s, d_st);
    hipLaunchKernelGGL(k_gicp_cov<false>, dim3((max_c + 255) / 256, n, 2), dim3(256), 0, s, d_tab, pts, cov, (int*)nullptr);
    for (int done = 0; done < run.max_it;) {  // setMaximumIterations; finished states skip their rounds
        const int rounds = run.max_it - done < ROUNDS_PER_CHUNK ? run.max_it - done : ROUNDS_PER_CHUNK;
        for (int it = 0; it < rounds; ++it) {
            hipLaunchKernelGGL(k_gicp_corr, dim3((max_src + 255) / 256, n), dim3(256), 0, s, d_tab, pts, cov, d_st, corr, maha, run.gate2);
            hipLaunchKernelGGL(k_gicp_bfgs, dim3(n), dim3(BF_THREADS), 0, s, d_tab, pts, corr, maha, d_st, run);
        }
        MML_HIP(hipGetLastError());
        MML_HIP(hipMemcpyAsync(h_st, d_st, sizeof(GicpState) * (size_t)n, hipMemcpyDeviceToHost, s));
        MML_HIP(hipStreamSynchronize(s));
        done += rounds;
        bool busy = false;  // (the state of a problem that does not align -- n_src = 0 -- is never advanced: nr stays 0)
        for (int i = 0; i < n && !busy; ++i) busy = !(h_st[i].converged || h_st[i].failed) && h_st[i].nr == done;
        if (!busy) break;
    }
    return MML_OK;
}

// what the caller sees of problem P: T written only on convergence, info zeroed for a problem that did not align
void gicp_result(const GicpProb& P, const GicpState& h, float* T, int* converged, mml_gicp_info* info) {
    *converged = 0;
    if (info) memset(info, 0, sizeof(*info));
    if (P.n_src == 0) return;
    *converged = (h.converged && !h.failed) ? 1 : 0;
    if (*converged) memcpy(T, h.T, sizeof(float) * 16);
    if (info) {
        info->outer_iterations = h.nr;
        info->objective_evaluations = h.evals;
        info->objective = h.fobj;
        info->n_source = P.n_src;
        info->n_target = P.n_tgt;
    }
}

// The n alignments of mml_gicp_align_batch; mml_gicp_align is its n = 1 case.  `who`: the entry point the caller used, which
// is the name a refusal carries.
int gicp_align_n(mml_ctx* ctx, const char* who, const GicpRun& run, int n, const float* src_xyz, const int* src_offsets, const float* tgt_xyz,
                 const int* tgt_offsets, float* T_inout, int* converged, mml_gicp_info* info) {
    if (n < 1 || n > MML_GICP_BATCH_MAX) return mml_refuse(ctx, MML_ERR_INVALID, "%s: n = %d is outside 1 .. %d", who, n, MML_GICP_BATCH_MAX);
    if (!(src_offsets && tgt_offsets && T_inout && converged)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null argument", who);
    if (src_offsets[0] < 0 || tgt_offsets[0] < 0) return mml_refuse(ctx, MML_ERR_INVALID, "%s: problem 0: a negative offset", who);
    for (int i = 0; i < n; ++i)
        if (src_offsets[i + 1] < src_offsets[i] || tgt_offsets[i + 1] < tgt_offsets[i])
            return mml_refuse(ctx, MML_ERR_INVALID, "%s: problem %d: its clouds end before their start (offsets must not decrease)", who, i);
    if ((src_offsets[n] > src_offsets[0] && !src_xyz) || (tgt_offsets[n] > tgt_offsets[0] && !tgt_xyz))
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null cloud", who);
    int rc = mml_enter_idle(ctx);
    if (rc != MML_OK) return rc;
    std::vector<GicpProb> tab((size_t)n);
    size_t n_pts = 0, n_srcs = 0;
    int max_src = 0, max_tgt = 0;
    for (int i = 0; i < n; ++i) {
        place_problem(tab[i], src_offsets[i + 1] - src_offsets[i], tgt_offsets[i + 1] - tgt_offsets[i], n_pts, n_srcs);
        max_src = tab[i].n_src > max_src ? tab[i].n_src : max_src;
        max_tgt = tab[i].n_tgt > max_tgt ? tab[i].n_tgt : max_tgt;
    }
    if (n_pts > 0x7fffffffull) return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: %zu points in one call", who, n_pts);
    const GicpIo io((size_t)n, n_pts);
    const GicpBig big(n_pts, n_srcs, false);
    MmlGicpDev* d = mml_side<MmlGicpDev>(ctx, MML_SIDE_GICP);
    if (n_pts > 0 && (d->io.reserve(ctx, io.bytes) || d->big.reserve(ctx, big.bytes))) return MML_ERR_HIP;
    GicpState* h_st = nullptr;
    if (n_pts > 0) {
        hipStream_t s = MML_STREAM(ctx);
        char *h = d->io.h, *g = d->io.d;
        memcpy(io.tab.in(h), tab.data(), io.tab.bytes());
        float4* hp = io.pts.in(h);
        for (int i = 0; i < n; ++i) {
            const GicpProb& P = tab[i];
            const float* a = src_xyz + 3 * (size_t)src_offsets[i];
            const float* b = tgt_xyz + 3 * (size_t)tgt_offsets[i];
            for (int k = 0; k < P.n_src; ++k) hp[P.src + k] = make_float4(a[3 * k], a[3 * k + 1], a[3 * k + 2], 0.f);
            for (int k = 0; k < P.n_tgt; ++k) hp[P.tgt + k] = make_float4(b[3 * k], b[3 * k + 1], b[3 * k + 2], 0.f);
        }
        MML_HIP(hipMemcpyAsync(io.tab.in(g), io.tab.in(h), io.tab.bytes(), hipMemcpyHostToDevice, s));
        MML_HIP(hipMemcpyAsync(io.pts.in(g), io.pts.in(h), io.pts.bytes(), hipMemcpyHostToDevice, s));
        h_st = io.st.in(h);
        rc = gicp_core(ctx, run, n, max_src, max_tgt, io.tab.in(g), io.pts.in(g), big.cov.in(d->big.d), big.maha.in(d->big.d),
                       big.corr.in(d->big.d), io.st.in(g), h_st);
        if (rc != MML_OK) return rc;
    }
    const GicpState none = {};
    for (int i = 0; i < n; ++i) gicp_result(tab[i], h_st ? h_st[i] : none, T_inout + 16 * (size_t)i, converged + i, info ? info + i : nullptr);
    return MML_OK;
}

}  // namespace

extern "C" int mml_gicp_align_batch(mml_ctx* ctx, int n, const float* src_xyz, const int* src_offsets, const float* tgt_xyz,
                                    const int* tgt_offsets, float* T_inout, int* converged, mml_gicp_info* info) {
    if (!ctx) return MML_ERR_INVALID;
    return gicp_align_n(ctx, "mml_gicp_align_batch", FEATURE_NODE_RUN, n, src_xyz, src_offsets, tgt_xyz, tgt_offsets, T_inout, converged, info);
}

extern "C" int mml_gicp_align(mml_ctx* ctx, const float* src_xyz, int n_src, const float* tgt_xyz, int n_tgt, float* T_inout, int* converged,
                              mml_gicp_info* info) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n_src >= 0 && n_tgt >= 0 && (n_src == 0 || src_xyz) && (n_tgt == 0 || tgt_xyz) && T_inout && converged, MML_ERR_INVALID,
                "bad arguments");
    const int so[2] = {0, n_src}, to[2] = {0, n_tgt};
    return gicp_align_n(ctx, "mml_gicp_align", FEATURE_NODE_RUN, 1, src_xyz, so, tgt_xyz, to, T_inout, converged, info);
}

namespace {

// the caller's settings as the kernels take them; a refusal before any device work
int gicp_run_of(mml_ctx* ctx, const char* who, const mml_gicp_opts* o, GicpRun& run) {
    if (!o) return mml_refuse(ctx, MML_ERR_INVALID, "%s: null options", who);
    if (o->max_iterations < 1) return mml_refuse(ctx, MML_ERR_INVALID, "%s: max_iterations = %d is below 1", who, o->max_iterations);
    if (!(isfinite(o->transformation_epsilon) && o->transformation_epsilon > 0.0))
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: transformation_epsilon = %g is not a positive finite number", who, o->transformation_epsilon);
    if (isnan(o->max_correspondence_distance)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: max_correspondence_distance is NaN", who);
    run.max_it = o->max_iterations;
    run.inv_trans_eps = 1.0 / o->transformation_epsilon;
    run.gate2 = o->max_correspondence_distance > 0.0 ? o->max_correspondence_distance * o->max_correspondence_distance : 0.0;
    return MML_OK;
}

}  // namespace

extern "C" int mml_gicp_align_opts(mml_ctx* ctx, const float* src_xyz, int n_src, const float* tgt_xyz, int n_tgt, const mml_gicp_opts* opts,
                                   float* T_inout, int* converged, mml_gicp_info* info) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n_src >= 0 && n_tgt >= 0 && (n_src == 0 || src_xyz) && (n_tgt == 0 || tgt_xyz) && T_inout && converged, MML_ERR_INVALID,
                "bad arguments");
    GicpRun run;
    const int rc = gicp_run_of(ctx, "mml_gicp_align_opts", opts, run);
    if (rc != MML_OK) return rc;
    const int so[2] = {0, n_src}, to[2] = {0, n_tgt};
    return gicp_align_n(ctx, "mml_gicp_align_opts", run, 1, src_xyz, so, tgt_xyz, to, T_inout, converged, info);
}

// mml_gicp_align_opts on two clouds that are on the device already (calibrate.hip), on an idle context: the clouds are copied
// device to device into the alignments' own block.  (x, y, z are read; w travels along unused.)
int mml_gicp_align_device(mml_ctx* ctx, const char* who, const float4* d_src, int n_src, const float4* d_tgt, int n_tgt,
                          const mml_gicp_opts* opts, float* T_inout, int* converged, mml_gicp_info* info) {
    GicpRun run;
    int rc = gicp_run_of(ctx, who, opts, run);
    if (rc != MML_OK) return rc;
    GicpProb P;
    size_t n_pts = 0, n_srcs = 0;
    place_problem(P, n_src, n_tgt, n_pts, n_srcs);
    const GicpState none = {};
    const GicpState* h_st = &none;
    if (n_pts > 0) {
        const GicpIo io(1, 0);
        const GicpBig big(n_pts, n_srcs, true);
        MmlGicpDev* d = mml_side<MmlGicpDev>(ctx, MML_SIDE_GICP);
        if (d->io.reserve(ctx, io.bytes) || d->big.reserve(ctx, big.bytes)) return MML_ERR_HIP;
        hipStream_t s = MML_STREAM(ctx);
        char *h = d->io.h, *g = d->io.d;
        memcpy(io.tab.in(h), &P, sizeof(P));
        float4* pts = big.pts.in(d->big.d);
        MML_HIP(hipMemcpyAsync(io.tab.in(g), io.tab.in(h), io.tab.bytes(), hipMemcpyHostToDevice, s));
        MML_HIP(hipMemcpyAsync(pts + P.src, d_src, sizeof(float4) * (size_t)n_src, hipMemcpyDeviceToDevice, s));
        MML_HIP(hipMemcpyAsync(pts + P.tgt, d_tgt, sizeof(float4) * (size_t)n_tgt, hipMemcpyDeviceToDevice, s));
        rc = gicp_core(ctx, run, 1, P.n_src, P.n_tgt, io.tab.in(g), pts, big.cov.in(d->big.d), big.maha.in(d->big.d), big.corr.in(d->big.d),
                       io.st.in(g), io.st.in(h));
        if (rc != MML_OK) return rc;
        h_st = io.st.in(h);
    }
    gicp_result(P, *h_st, T_inout, converged, info);
    return MML_OK;
}

namespace {

// The refresh of mml_gicp_refresh_batch; mml_gicp_refresh is its count = 1, chain = 0 case.  `who` as in gicp_align_n.
int gicp_refresh_n(mml_ctx* ctx, const char* who, int first_slot, int count, float* extrinsics, int chain, int apply, int* refreshed,
                   mml_gicp_info* info) {
    if (count < 1 || count > MML_GICP_BATCH_MAX)
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: count = %d is outside 1 .. %d", who, count, MML_GICP_BATCH_MAX);
    if (first_slot < 0 || first_slot >= ctx->B)
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: slot %d is outside the context's 0 .. %d", who, first_slot, ctx->B - 1);
    if (count > ctx->B - first_slot)
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: slot %d is outside the context's 0 .. %d", who, ctx->B, ctx->B - 1);
    if (!extrinsics) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null argument", who);
    int rc = mml_enter_idle(ctx);
    if (rc != MML_OK) return rc;
    // (the gather and the apply below read and rewrite ln_pts / ln_label.  A partly undistorted slot carries the "undistorted" flag
    //  and is refused further down; it is settled all the same, so that no path into those kernels depends on that refusal)
    rc = mml_cloud_settle(ctx, first_slot, count);
    if (rc != MML_OK) return rc;
    hipStream_t s = MML_STREAM(ctx);
    const size_t n = (size_t)count, f = (size_t)first_slot;
    const GicpIo io(n, 0);
    MmlGicpDev* d = mml_side<MmlGicpDev>(ctx, MML_SIDE_GICP);
    if (d->io.reserve(ctx, io.bytes)) return MML_ERR_HIP;
    char *h = d->io.h, *g = d->io.d;
    // counters, valid points per sensor region of the slots' storage, the slots' state flags
    const int *fi = io.fi.in(h), *cb = io.cb.in(h), *fl = io.fl.in(h);
    MML_HIP(hipMemcpyAsync(io.fi.in(h), ctx->fu_info + 8 * f, io.fi.bytes(), hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(io.cb.in(h), ctx->cb_n + 2 * f, io.cb.bytes(), hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(io.fl.in(h), ctx->slot_flags + 2 * f, io.fl.bytes(), hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < count; ++i) {
        // the refresh belongs to the feature node: it aligns the surf clouds of the EXTRACTED scan (raw coordinates, raw order)
        if ((fl[2 * i] & 3) != 0)
            return mml_refuse(ctx, MML_ERR_STATE, "%s: slot %d holds an uploaded or undistorted cloud (call it after mml_extract, before mml_undistort)",
                              who, first_slot + i);
        // (the one-pass bucketing keeps no per-point line ids; they are re-derived below from the slot's RAW buffers, which must
        //  therefore still be the ones the extraction read -- not a scan staged early for the next call)
        if (!ctx->raw_extracted[first_slot + i])
            return mml_refuse(ctx, MML_ERR_STATE, "%s: slot %d's raw scan was re-uploaded after mml_extract (or never extracted)", who, first_slot + i);
    }
    std::vector<GicpProb> tab(n);
    memset(tab.data(), 0, sizeof(GicpProb) * n);
    int n_go = 0, go_lo = count, go_hi = -1;  // the frames that are not skipped, and the first and last of them
    for (int i = 0; i < count; ++i)
        if (fi[8 * i + 4] > 100) {  // union_msg.livox_corner_num > 100 (unionFeatureExtract.cpp:302)
            ++n_go;
            go_lo = i < go_lo ? i : go_lo;
            go_hi = i;
        }
    const GicpState* h_st = nullptr;
    size_t n_pts = 0, n_srcs = 0;
    if (n_go > 0) {
        GatherArgs A{ctx->raw_line, ctx->d_n_in, ctx->seg_flat, ctx->seg_flat_n, ctx->fu_info, ctx->ln_label, ctx->ln_pts,
                     first_slot,    ctx->NT,     ctx->NV,       ctx->onepass ? MML_OP_BLK : (1 << 30)};
        // (the one-pass bucketing keeps no per-point line ids: they are recomputed in one launch, for the slots from the first
        //  to the last frame that aligns.  A skipped slot between them has its raw_line / raw_ori / blk_cnt rewritten too: with
        //  the values they already hold, since they are a function of the slot's raw scan alone, which raw_extracted pins)
        if (ctx->onepass) {
            rc = mml_launch_raw_lines(ctx, first_slot + go_lo, go_hi - go_lo + 1);
            if (rc != MML_OK) return rc;
        }
        hipLaunchKernelGGL(k_gicp_gather_raw, dim3(2, count), dim3(RG_THREADS), 0, s, A, (const GicpProb*)nullptr, (float4*)nullptr,
                           io.cnt.in(g));
        MML_HIP(hipGetLastError());
        MML_HIP(hipMemcpyAsync(io.cnt.in(h), io.cnt.in(g), io.cnt.bytes(), hipMemcpyDeviceToHost, s));
        MML_HIP(hipStreamSynchronize(s));
        const int* cnt = io.cnt.in(h);
        int max_src = 0, max_tgt = 0;
        for (int i = 0; i < count; ++i) {  // source: Livox surf, target: Velodyne surf (:307)
            place_problem(tab[i], cnt[2 * i + 1], cnt[2 * i], n_pts, n_srcs);
            max_src = tab[i].n_src > max_src ? tab[i].n_src : max_src;
            max_tgt = tab[i].n_tgt > max_tgt ? tab[i].n_tgt : max_tgt;
        }
        if (n_pts > 0x7fffffffull) return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: %zu surf points in one call", who, n_pts);
        if (n_pts > 0) {
            const GicpBig big(n_pts, n_srcs, true);
            if (d->big.reserve(ctx, big.bytes)) return MML_ERR_HIP;  // (no slot has been touched yet)
            memcpy(io.tab.in(h), tab.data(), io.tab.bytes());
            MML_HIP(hipMemcpyAsync(io.tab.in(g), io.tab.in(h), io.tab.bytes(), hipMemcpyHostToDevice, s));
            const GicpProb* d_tab = io.tab.in(g);
            float4* pts = big.pts.in(d->big.d);
            hipLaunchKernelGGL(k_gicp_gather_raw, dim3(2, count), dim3(RG_THREADS), 0, s, A, d_tab, pts, (int*)nullptr);
            GicpState* hs = io.st.in(h);
            rc = gicp_core(ctx, FEATURE_NODE_RUN, count, max_src, max_tgt, d_tab, pts, big.cov.in(d->big.d), big.maha.in(d->big.d), big.corr.in(d->big.d), io.st.in(g),
                           hs);
            if (rc != MML_OK) return rc;
            h_st = hs;
        }
    }
    // extri_mtx through the frames: a frame that converged replaces it, every other frame keeps what the frame before it left
    // (chained), or its own row (not chained)
    const GicpState none = {};
    float* h_mat = io.mat.in(h);
    int* h_napp = io.napp.in(h);
    int max_app = 0;
    for (int i = 0; i < count; ++i) {
        float* row = extrinsics + 16 * (size_t)i;
        if (chain && i > 0) memcpy(row, row - 16, sizeof(float) * 16);
        int conv = 0;
        gicp_result(tab[i], h_st ? h_st[i] : none, row, &conv, info ? info + i : nullptr);
        if (refreshed) refreshed[i] = conv;
        // pcl::transformPointCloud(*livoCombinePtr, *livoCombinePtr, extri_mtx) (:312): the Livox region, of a frame that was not skipped
        h_napp[i] = (apply && fi[8 * i + 4] > 100) ? cb[2 * i + 1] : 0;
        memcpy(h_mat + 16 * (size_t)i, row, sizeof(float) * 16);
        max_app = h_napp[i] > max_app ? h_napp[i] : max_app;
    }
    if (max_app > 0) {
        // matrices | point counts: one copy, up to the field behind them
        MML_HIP(hipMemcpyAsync(io.mat.in(g), io.mat.in(h), io.fi.off - io.mat.off, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_gicp_apply, dim3((max_app + 255) / 256, count), dim3(256), 0, s, ctx->ln_pts, first_slot, ctx->NT, ctx->NV,
                           io.napp.in(g), io.mat.in(g));
        MML_HIP(hipGetLastError());
        MML_HIP(hipStreamSynchronize(s));
    }
    return MML_OK;
}

}  // namespace

extern "C" int mml_gicp_refresh_batch(mml_ctx* ctx, int first_slot, int count, float* extrinsics, int chain, int apply, int* refreshed,
                                      mml_gicp_info* info) {
    if (!ctx) return MML_ERR_INVALID;
    return gicp_refresh_n(ctx, "mml_gicp_refresh_batch", first_slot, count, extrinsics, chain, apply, refreshed, info);
}

extern "C" int mml_gicp_refresh(mml_ctx* ctx, int slot, float* extrinsic_inout, int apply, int* refreshed, mml_gicp_info* info) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(slot >= 0 && slot < ctx->B && extrinsic_inout, MML_ERR_INVALID, "bad arguments");
    if (refreshed) *refreshed = 0;
    if (info) memset(info, 0, sizeof(*info));
    return gicp_refresh_n(ctx, "mml_gicp_refresh", slot, 1, extrinsic_inout, 0, apply, refreshed, info);
}

// ---- test hook: the kernels and __device__ functions above on caller-supplied inputs (mml_debug_gicp) ---------------------------
namespace {

// MML_GICP_DBG_EVAL: one workgroup as k_gicp_bfgs forms it, gicp_eval at K states one after the other; every lane holds the same f
// and g, lane 0 and lane BF_THREADS - 1 each write their own copy (out: K x 2 x 7)
__global__ __launch_bounds__(BF_THREADS) void k_gicp_dbg_eval(const float4* src, const float4* tgt, const int* corr, const double* maha, int n,
                                                             int m, int gated, const double* xs, int K, int grad, double* out) {
    __shared__ double s_terms[13 * EV_ROW];
    __shared__ double s_tot[13];
    __shared__ int s_keep[EV_CH];
    EvalCtx E{src, tgt, corr, maha, n, m, s_terms, s_tot, gated ? s_keep : nullptr};
    for (int k = 0; k < K; ++k) {
        double x[6], g[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 6; ++i) x[i] = xs[6 * k + i];
        const double f = gicp_eval(E, x, grad ? g : nullptr);
        if (threadIdx.x == 0 || threadIdx.x == BF_THREADS - 1) {
            double* o = out + 7 * (size_t)(2 * k + (threadIdx.x != 0));
            o[0] = f;
#pragma unroll
            for (int i = 0; i < 6; ++i) o[1 + i] = g[i];
        }
    }
}

// MML_GICP_DBG_INTERP / _QUAD / _STATE: one lane per item
__global__ void k_gicp_dbg_scalar(int op, const double* in, int n, double* out_d, float* out_f) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op == MML_GICP_DBG_INTERP) {
        const double* a = in + 8 * (size_t)i;
        out_d[i] = interpolate(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
    } else if (op == MML_GICP_DBG_QUAD) {
        const double* a = in + 3 * (size_t)i;
        double x0 = 0, x1 = 0;
        const int cnt = solve_quadratic(a[0], a[1], a[2], x0, x1);
        out_d[3 * (size_t)i] = (double)cnt;
        out_d[3 * (size_t)i + 1] = x0;
        out_d[3 * (size_t)i + 2] = x1;
    } else {
        float T[16];
        double x[6];
        apply_state(in + 6 * (size_t)i, T);
        state_of(T, x);
#pragma unroll
        for (int c = 0; c < 16; ++c) out_f[16 * (size_t)i + c] = T[c];
#pragma unroll
        for (int c = 0; c < 6; ++c) out_d[6 * (size_t)i + c] = x[c];
    }
}

template <class T>
bool dbg_up(MmlTemp<T>& b, const void* h, size_t n) {
    return b.alloc(n ? n : 1) == hipSuccess && (n == 0 || hipMemcpy(b.d, h, sizeof(T) * n, hipMemcpyHostToDevice) == hipSuccess);
}
template <class T>
bool dbg_zero(MmlTemp<T>& b, size_t n) {
    return b.alloc(n ? n : 1) == hipSuccess && hipMemset(b.d, 0, sizeof(T) * (n ? n : 1)) == hipSuccess;
}
template <class T>
bool dbg_down(void* h, const MmlTemp<T>& b, size_t n) {
    return hipMemcpy(h, b.d, sizeof(T) * n, hipMemcpyDeviceToHost) == hipSuccess;
}
// source | target as the kernels' packed float4 array
std::vector<float4> dbg_pack(const float* src, int ns, const float* tgt, int nt) {
    std::vector<float4> p((size_t)ns + nt);
    for (int k = 0; k < ns; ++k) p[k] = make_float4(src[3 * k], src[3 * k + 1], src[3 * k + 2], 0.f);
    for (int k = 0; k < nt; ++k) p[(size_t)ns + k] = make_float4(tgt[3 * k], tgt[3 * k + 1], tgt[3 * k + 2], 0.f);
    return p;
}

}  // namespace

extern "C" int mml_debug_gicp(mml_ctx* ctx, int op, const mml_gicp_debug* io) {
    if (!ctx) return MML_ERR_INVALID;
    const char* who = "mml_debug_gicp";
    if (!io) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null argument", who);
    if (op < MML_GICP_DBG_COV || op > MML_GICP_DBG_ROUND) return mml_refuse(ctx, MML_ERR_INVALID, "%s: op = %d is outside 0 .. 6", who, op);
    const int ns = io->n_src, nt = io->n_tgt, K = io->k;
    const bool gated = io->gate2 > 0.0;
    // ---- every refusal, before anything is allocated or launched ----
    if (op == MML_GICP_DBG_COV) {
        if (nt < GK || nt > MML_GICP_DBG_MAX_POINTS)
            return mml_refuse(ctx, MML_ERR_INVALID, "%s: COV: n = %d is outside %d .. %d", who, nt, GK, MML_GICP_DBG_MAX_POINTS);
        if (!(io->tgt && io->out_d && io->out_i)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: COV: a null argument", who);
    } else if (op == MML_GICP_DBG_CORR || op == MML_GICP_DBG_EVAL || op == MML_GICP_DBG_ROUND) {
        if (ns < 1 || nt < 1 || ns > MML_GICP_DBG_MAX_POINTS || nt > MML_GICP_DBG_MAX_POINTS)
            return mml_refuse(ctx, MML_ERR_INVALID, "%s: clouds of %d and %d points (1 .. %d each)", who, ns, nt, MML_GICP_DBG_MAX_POINTS);
        if (!(io->src && io->tgt)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null cloud", who);
        if (isnan(io->gate2)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: gate2 is NaN", who);
        if (op == MML_GICP_DBG_CORR) {
            if (!(io->cov_src && io->cov_tgt && io->T && io->out_i && io->out_d)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: CORR: a null argument", who);
        } else {
            if (!(io->corr && io->maha)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null correspondence list", who);
            // a hole (corr = -1) only with a gate, as k_gicp_corr leaves them; every other entry inside the target
            for (int i = 0; i < ns; ++i)
                if (io->corr[i] >= nt || io->corr[i] < (gated ? -1 : 0))
                    return mml_refuse(ctx, MML_ERR_INVALID, "%s: corr[%d] = %d is outside the target of %d points%s", who, i, io->corr[i], nt,
                                      gated ? "" : " (holes need gate2 > 0)");
            if (op == MML_GICP_DBG_EVAL) {
                int kept = 0;
                for (int i = 0; i < ns; ++i) kept += io->corr[i] >= 0;
                if (kept < 1) return mml_refuse(ctx, MML_ERR_INVALID, "%s: EVAL: no correspondence", who);
                if (K < 1 || K > MML_GICP_DBG_MAX_ITEMS) return mml_refuse(ctx, MML_ERR_INVALID, "%s: EVAL: K = %d is outside 1 .. %d", who, K, MML_GICP_DBG_MAX_ITEMS);
                if (!(io->x && io->out_d)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: EVAL: a null argument", who);
            } else {
                if (!(io->T && io->out_f && io->out_i && io->out_d)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: ROUND: a null argument", who);
                if (io->max_iterations < 1 || !(isfinite(io->transformation_epsilon) && io->transformation_epsilon > 0.0))
                    return mml_refuse(ctx, MML_ERR_INVALID, "%s: ROUND: bad settings", who);
            }
        }
    } else {
        if (K < 1 || K > MML_GICP_DBG_MAX_ITEMS) return mml_refuse(ctx, MML_ERR_INVALID, "%s: n = %d items is outside 1 .. %d", who, K, MML_GICP_DBG_MAX_ITEMS);
        if (!(io->x && io->out_d) || (op == MML_GICP_DBG_STATE && !io->out_f)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null argument", who);
    }
    int rc = mml_enter_idle(ctx);
    if (rc != MML_OK) return rc;
    hipStream_t s = MML_STREAM(ctx);
    bool ok = true;
    if (op == MML_GICP_DBG_INTERP || op == MML_GICP_DBG_QUAD || op == MML_GICP_DBG_STATE) {
        const size_t wi = op == MML_GICP_DBG_INTERP ? 8 : op == MML_GICP_DBG_QUAD ? 3 : 6, wo = op == MML_GICP_DBG_INTERP ? 1 : op == MML_GICP_DBG_QUAD ? 3 : 6;
        MmlTemp<double> in, od;
        MmlTemp<float> of;
        ok = dbg_up(in, io->x, wi * K) && dbg_zero(od, wo * K) && dbg_zero(of, 16 * (size_t)K);
        if (ok) {
            hipLaunchKernelGGL(k_gicp_dbg_scalar, dim3((K + 255) / 256), dim3(256), 0, s, op, in.d, K, od.d, of.d);
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        }
        ok = ok && dbg_down(io->out_d, od, wo * K) && (op != MML_GICP_DBG_STATE || dbg_down(io->out_f, of, 16 * (size_t)K));
        return ok ? MML_OK : MML_ERR_HIP;
    }
    if (op == MML_GICP_DBG_COV) {  // a one-problem table: the cloud as the target (blockIdx.z = 0), no source
        GicpProb P;
        memset(&P, 0, sizeof(P));
        P.n_tgt = nt;
        const std::vector<float4> hp = dbg_pack(nullptr, 0, io->tgt, nt);
        MmlTemp<GicpProb> tab;
        MmlTemp<float4> pts;
        MmlTemp<double> cov;
        MmlTemp<int> ids;
        ok = dbg_up(tab, &P, 1) && dbg_up(pts, hp.data(), hp.size()) && dbg_zero(cov, 9 * (size_t)nt) && dbg_zero(ids, GK * (size_t)nt);
        if (ok) {
            hipLaunchKernelGGL(k_gicp_cov<true>, dim3((nt + 255) / 256, 1, 1), dim3(256), 0, s, tab.d, pts.d, cov.d, ids.d);
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        }
        ok = ok && dbg_down(io->out_d, cov, 9 * (size_t)nt) && dbg_down(io->out_i, ids, GK * (size_t)nt);
        return ok ? MML_OK : MML_ERR_HIP;
    }
    // CORR / EVAL / ROUND: source then target, as place_problem lays a problem out
    GicpProb P;
    memset(&P, 0, sizeof(P));
    P.src = 0;
    P.tgt = ns;
    P.n_src = ns;
    P.n_tgt = nt;
    const std::vector<float4> hp = dbg_pack(io->src, ns, io->tgt, nt);
    MmlTemp<GicpProb> tab;
    MmlTemp<float4> pts;
    MmlTemp<double> maha;
    MmlTemp<int> corr;
    MmlTemp<GicpState> st;
    ok = dbg_up(tab, &P, 1) && dbg_up(pts, hp.data(), hp.size());
    GicpState h_st;
    memset(&h_st, 0, sizeof(h_st));
    if (io->T) memcpy(h_st.T, io->T, sizeof(float) * 16);
    ok = ok && dbg_up(st, &h_st, 1);
    if (op == MML_GICP_DBG_CORR) {
        std::vector<double> hc(9 * ((size_t)ns + nt));
        memcpy(hc.data(), io->cov_src, sizeof(double) * 9 * (size_t)ns);
        memcpy(hc.data() + 9 * (size_t)ns, io->cov_tgt, sizeof(double) * 9 * (size_t)nt);
        MmlTemp<double> cov;
        ok = ok && dbg_up(cov, hc.data(), hc.size()) && dbg_zero(maha, 9 * (size_t)ns) && dbg_zero(corr, (size_t)ns);
        if (ok) {
            hipLaunchKernelGGL(k_gicp_corr, dim3((ns + 255) / 256, 1), dim3(256), 0, s, tab.d, pts.d, cov.d, st.d, corr.d, maha.d, gated ? io->gate2 : 0.0);
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        }
        ok = ok && dbg_down(io->out_i, corr, (size_t)ns) && dbg_down(io->out_d, maha, 9 * (size_t)ns);
        return ok ? MML_OK : MML_ERR_HIP;
    }
    ok = ok && dbg_up(corr, io->corr, (size_t)ns) && dbg_up(maha, io->maha, 9 * (size_t)ns);
    if (op == MML_GICP_DBG_EVAL) {
        int m = 0;  // as k_gicp_bfgs counts it: every point without a gate, the kept ones with
        for (int i = 0; i < ns; ++i) m += io->corr[i] >= 0;
        MmlTemp<double> xs, out;
        ok = ok && dbg_up(xs, io->x, 6 * (size_t)K) && dbg_zero(out, 14 * (size_t)K);
        if (ok) {
            hipLaunchKernelGGL(k_gicp_dbg_eval, dim3(1), dim3(BF_THREADS), 0, s, pts.d, pts.d + ns, corr.d, maha.d, ns, m, gated ? 1 : 0, xs.d, K,
                               io->grad ? 1 : 0, out.d);
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        }
        ok = ok && dbg_down(io->out_d, out, 14 * (size_t)K);
        return ok ? MML_OK : MML_ERR_HIP;
    }
    const GicpRun run = {io->max_iterations, 1.0 / io->transformation_epsilon, gated ? io->gate2 : 0.0};
    if (ok) {
        hipLaunchKernelGGL(k_gicp_bfgs, dim3(1), dim3(BF_THREADS), 0, s, tab.d, pts.d, corr.d, maha.d, st.d, run);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    }
    ok = ok && dbg_down(&h_st, st, 1);
    if (!ok) return MML_ERR_HIP;
    memcpy(io->out_f, h_st.T, sizeof(float) * 16);
    io->out_i[0] = h_st.converged;
    io->out_i[1] = h_st.failed;
    io->out_i[2] = h_st.nr;
    io->out_i[3] = h_st.evals;
    io->out_d[0] = h_st.fobj;
    io->out_d[1] = h_st.delta;
    return MML_OK;
}
