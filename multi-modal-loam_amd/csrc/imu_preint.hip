// imu_preint.hip -- mml_imu_preintegrate_batch: IMUIntegrator::PreIntegration (IMUIntegrator.cpp:108-166) for n intervals in one
// call.  The arithmetic is imu_preint.h, one routine for both sides: a NULL context runs its host build in a loop, a context
// runs k_imu_preintegrate, one workgroup of one wavefront per interval -- Jacobian, covariance and the per-sample blocks stay
// in LDS for the whole chain over the samples (13.0 KB, so twelve intervals are resident on a CU) and are written once at the
// end.  One upload (offsets | biases | samples from one pinned block), one launch, one read-back.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "imu_preint.h"
#include "mml_internal.h"

namespace {

__global__ __launch_bounds__(64) void k_imu_preintegrate(const double* samples, const int* offsets, const double* bias /* n x (bg | ba) */,
                                                         mml_imu_preint* out) {
    __shared__ PreintWork s_work;
    const size_t i = blockIdx.x;
    const int s0 = offsets[i], cnt = offsets[i + 1] - s0;
    imu_preint_interval(samples + 7 * (size_t)s0, cnt, bias + 6 * i, bias + 6 * i + 3, out + i, s_work);
}

}  // namespace

struct MmlPreintDev {  // device and pinned buffers, sized for the largest call seen
    size_t in_cap = 0;  // bytes
    int out_cap = 0;    // intervals
    char* d_in = nullptr;
    char* h_in = nullptr;  // pinned
    mml_imu_preint* d_out = nullptr;
    mml_imu_preint* h_out = nullptr;  // pinned
};

void mml_imu_preint_release(mml_ctx* ctx) {
    MmlPreintDev* d = ctx->preint;
    if (!d) return;
    if (d->d_in) hipFree(d->d_in);
    if (d->h_in) hipHostFree(d->h_in);
    if (d->d_out) hipFree(d->d_out);
    if (d->h_out) hipHostFree(d->h_out);
    delete d;
    ctx->preint = nullptr;
}

static int preint_reserve(mml_ctx* ctx, size_t in_bytes, int n) {
    if (!ctx->preint) ctx->preint = new MmlPreintDev();
    MmlPreintDev* d = ctx->preint;
    if (in_bytes > d->in_cap) {  // (every call drains the stream before it returns: nothing is in flight)
        if (d->d_in) hipFree(d->d_in);
        if (d->h_in) hipHostFree(d->h_in);
        d->d_in = d->h_in = nullptr;
        d->in_cap = 0;
        MML_HIP(hipMalloc(reinterpret_cast<void**>(&d->d_in), in_bytes));
        MML_HIP(hipHostMalloc(reinterpret_cast<void**>(&d->h_in), in_bytes, hipHostMallocDefault));
        d->in_cap = in_bytes;
    }
    if (n > d->out_cap) {
        if (d->d_out) hipFree(d->d_out);
        if (d->h_out) hipHostFree(d->h_out);
        d->d_out = d->h_out = nullptr;
        d->out_cap = 0;
        MML_HIP(hipMalloc(reinterpret_cast<void**>(&d->d_out), sizeof(mml_imu_preint) * n));
        MML_HIP(hipHostMalloc(reinterpret_cast<void**>(&d->h_out), sizeof(mml_imu_preint) * n, hipHostMallocDefault));
        d->out_cap = n;
    }
    return MML_OK;
}

// (a NULL context has nowhere to carry the message)
#define PREINT_REFUSE(cond, ...)                                        \
    do {                                                                \
        if (!(cond)) {                                                  \
            if (ctx) {                                                  \
                char m_[192];                                           \
                snprintf(m_, sizeof(m_), "mml_imu_preintegrate_batch: " __VA_ARGS__); \
                ctx->err = m_;                                          \
            }                                                           \
            return MML_ERR_INVALID;                                     \
        }                                                               \
    } while (0)

extern "C" int mml_imu_preintegrate_batch(mml_ctx* ctx, int n, const double* samples, const int* offsets, const double* bg,
                                          const double* ba, mml_imu_preint* out) {
    PREINT_REFUSE(n >= 1 && n <= MML_PREINT_BATCH_MAX, "n = %d is outside 1 .. %d", n, MML_PREINT_BATCH_MAX);
    PREINT_REFUSE(offsets && bg && ba && out, "a null argument");
    PREINT_REFUSE(offsets[0] == 0, "interval 0: offsets[0] is %d, not 0", offsets[0]);
    for (int i = 0; i < n; ++i)
        PREINT_REFUSE(offsets[i + 1] >= offsets[i], "interval %d: its end %d lies before its start %d", i, offsets[i + 1], offsets[i]);
    PREINT_REFUSE(samples || offsets[n] == 0, "samples is null");
    if (!ctx) {  // the host build of the routine
        PreintWork work;
        for (int i = 0; i < n; ++i)
            imu_preint_interval(samples + 7 * (size_t)offsets[i], offsets[i + 1] - offsets[i], bg + 3 * (size_t)i, ba + 3 * (size_t)i, out + i, work);
        return MML_OK;
    }
    MML_HIP(hipSetDevice(ctx->device));
    const size_t total = (size_t)offsets[n];
    const size_t off_bytes = (sizeof(int) * ((size_t)n + 1) + 7) & ~(size_t)7, bias_bytes = sizeof(double) * 6 * (size_t)n;
    const size_t in_bytes = off_bytes + bias_bytes + sizeof(double) * 7 * total;
    {
        const int rc = preint_reserve(ctx, in_bytes, n);
        if (rc != MML_OK) return rc;
    }
    MmlPreintDev* d = ctx->preint;
    memcpy(d->h_in, offsets, sizeof(int) * ((size_t)n + 1));
    double* h_bias = reinterpret_cast<double*>(d->h_in + off_bytes);
    for (int i = 0; i < n; ++i) {
        memcpy(h_bias + 6 * (size_t)i, bg + 3 * (size_t)i, sizeof(double) * 3);
        memcpy(h_bias + 6 * (size_t)i + 3, ba + 3 * (size_t)i, sizeof(double) * 3);
    }
    if (total) memcpy(d->h_in + off_bytes + bias_bytes, samples, sizeof(double) * 7 * total);
    hipStream_t s = MML_STREAM(ctx);
    MmlStageScope t(ctx, "imu_preintegrate");
    MML_HIP(hipMemcpyAsync(d->d_in, d->h_in, in_bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_imu_preintegrate, dim3(n), dim3(64), 0, s, reinterpret_cast<const double*>(d->d_in + off_bytes + bias_bytes),
                       reinterpret_cast<const int*>(d->d_in), reinterpret_cast<const double*>(d->d_in + off_bytes), d->d_out);
    MML_HIP(hipGetLastError());
    MML_HIP(hipMemcpyAsync(d->h_out, d->d_out, sizeof(mml_imu_preint) * n, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    memcpy(out, d->h_out, sizeof(mml_imu_preint) * n);
    return MML_OK;
}
