// marg_dense.h -- the dense tail of the marginalization (MarginalizationInfo::marginalize, ceresfunc.h:203-227), written
// once for the host (mml_fullwindow_marginalize, window_imu.hip) and the device (k_fw_marginalize / k_marg_dense,
// fullwindow_dev.hip): from the 30 x 30 system A, b of (frame 0 | frame 1) to the square-root prior J, r0 on frame 1.
//   Amm^-1 through the eigen-decomposition of the symmetric part of the marginalized block, eigenvalues <= 1e-8 dropped;
//   the Schur complement Ar = Arr - Arm Amm^-1 Amr, br = br - Arm Amm^-1 bm; J = sqrt(S) V^T, r0 = sqrt(S^-1) V^T br.
// The host build runs every loop below from 0 to its end on one thread.  The device build is called by ONE wavefront
// with A, b and the work space in LDS: a loop marked MARG_FOR has independent iterations and is spread over the lanes,
// a block marked MARG_LANE(l) is a sequential sum or search given to lane l, MARG_SYNC() orders the LDS traffic of the
// wavefront (no workgroup barrier).  Every element therefore receives the same operations in the same order on both
// sides -- sums over k ascending from 0.0, Jacobi rotations in (p, q) order with the scalars theta, t, c, s computed by
// every lane from the same values -- and with -ffp-contract=off and correctly rounded sqrt and / the two results are
// bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "imu_math.h"

namespace {

struct MargWork {  // four 15 x 15 matrices and the small vectors
    double M[4][225];
    double ev[15], br[15];
    double red[2];  // off / diag of a sweep
    int order[15];
};

#define MARG_HD __host__ __device__ __forceinline__  // (inlined: the device build then addresses its arguments as LDS)
#if defined(__HIP_DEVICE_COMPILE__)
#define MARG_FOR(e, n) for (int e = (int)(threadIdx.x & 63); e < (n); e += 64)
#define MARG_LANE(l) if ((int)(threadIdx.x & 63) == (l))
#define MARG_SYNC()                                               \
    do {                                                          \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    \
        __builtin_amdgcn_wave_barrier();                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");    \
    } while (0)
#else
#define MARG_FOR(e, n) for (int e = 0; e < (n); ++e)
#define MARG_LANE(l)
#define MARG_SYNC() \
    do {            \
    } while (0)
#endif

// cyclic Jacobi eigen-decomposition of the symmetric 15 x 15 matrix in A (destroyed): A = Vs diag(ev) Vs^T, eigenvalues
// ascending.  V: work space.
MARG_HD void marg_sym_eig15(double* A, double* V, double* Vs, double* ev, MargWork& w) {
    const int n = 15;
    MARG_FOR(e, 225) V[e] = (e / n == e % n) ? 1.0 : 0.0;
    MARG_SYNC();
    for (int sweep = 0; sweep < 100; ++sweep) {
        MARG_LANE(0) {
            double off = 0;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j)
                    if (i != j) off += A[i * n + j] * A[i * n + j];
            w.red[0] = off;
        }
        MARG_LANE(1) {
            double diag = 0;
            for (int i = 0; i < n; ++i) diag += A[i * n + i] * A[i * n + i];
            w.red[1] = diag;
        }
        MARG_SYNC();
        const double off = w.red[0], diag = w.red[1];
        if (off <= 1e-30 * diag || off == 0.0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                MARG_FOR(k, n) {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                }
                MARG_SYNC();  // the row loop sees the column loop's writes to the four pivot elements
                MARG_FOR(k, n) {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk;
                    A[q * n + k] = s * apk + c * aqk;
                }
                MARG_FOR(k, n) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
                MARG_SYNC();
            }
    }
    MARG_LANE(0) {  // ascending selection sort of the eigenvalues
        int* order = w.order;
        for (int i = 0; i < n; ++i) order[i] = i;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j)
                if (A[order[j] * n + order[j]] < A[order[i] * n + order[i]]) {
                    const int t = order[i];
                    order[i] = order[j];
                    order[j] = t;
                }
    }
    MARG_SYNC();
    MARG_FOR(e, 225) {
        const int r = e / n, c = e - n * r;
        Vs[e] = V[r * n + w.order[c]];
        if (r == 0) ev[c] = A[w.order[c] * n + w.order[c]];
    }
    MARG_SYNC();
}

// A: 30 x 30 row-major, b: 30 (the first 15 parameters are marginalized) -> J: 15 x 15 row-major, r0: 15
MARG_HD void marg_dense(const double* A, const double* b, double* J, double* r0, MargWork& w) {
    const int m = 15, n = 15, N = 30;
    const double eps = 1e-8;
    double *M0 = w.M[0], *M1 = w.M[1], *M2 = w.M[2], *M3 = w.M[3];
    // Amm^-1 through the eigen-decomposition of its symmetric part, eigenvalues <= eps dropped (:203-206)
    MARG_FOR(e, 225) {
        const int r = e / m, c = e - m * r;
        M0[e] = 0.5 * (A[r * N + c] + A[c * N + r]);
    }
    MARG_SYNC();
    marg_sym_eig15(M0, M1, M2, w.ev, w);  // V = M2
    double* Ainv = M3;
    MARG_FOR(e, 225) {
        const int r = e / m, c = e - m * r;
        double sum = 0;
        for (int k = 0; k < m; ++k)
            if (w.ev[k] > eps) sum += M2[r * m + k] * (1.0 / w.ev[k]) * M2[c * m + k];
        Ainv[e] = sum;
    }
    MARG_SYNC();
    // Schur complement (:208-214)
    double* T = M0;  // Arm * Amm_inv
    MARG_FOR(e, 225) {
        const int r = e / m, c = e - m * r;
        double sum = 0;
        for (int k = 0; k < m; ++k) sum += A[(m + r) * N + k] * Ainv[k * m + c];
        T[e] = sum;
    }
    MARG_SYNC();
    double* Ar = M1;
    MARG_FOR(e, 240) {
        if (e < 225) {
            const int r = e / n, c = e - n * r;
            double sum = 0;
            for (int k = 0; k < m; ++k) sum += T[r * m + k] * A[k * N + m + c];
            Ar[e] = A[(m + r) * N + m + c] - sum;
        } else {
            const int r = e - 225;
            double sb = 0;
            for (int k = 0; k < m; ++k) sb += T[r * m + k] * b[k];
            w.br[r] = b[m + r] - sb;
        }
    }
    MARG_SYNC();
    MARG_FOR(e, 225) {
        const int r = e / n, c = e - n * r;
        if (c > r) Ar[r * n + c] = Ar[c * n + r] = 0.5 * (Ar[r * n + c] + Ar[c * n + r]);
    }
    MARG_SYNC();
    // linearized_jacobians = sqrt(S) V^T, linearized_residuals = sqrt(S^-1) V^T b  (:216-227)
    marg_sym_eig15(Ar, M2, M3, w.ev, w);  // V2 = M3
    MARG_FOR(i, n) {
        const double sv = w.ev[i] > eps ? sqrt(w.ev[i]) : 0.0;
        const double si = w.ev[i] > eps ? sqrt(1.0 / w.ev[i]) : 0.0;
        double vb = 0;
        for (int k = 0; k < n; ++k) {
            J[i * 15 + k] = sv * M3[k * n + i];
            vb += M3[k * n + i] * w.br[k];
        }
        r0[i] = si * vb;
    }
    MARG_SYNC();
}

}  // namespace
