// imu_preint.hip -- mml_imu_preintegrate_batch: IMUIntegrator::PreIntegration (IMUIntegrator.cpp:108-166) for n intervals in one
// call.  The arithmetic is imu_preint.h, one routine for both sides: a NULL context runs its host build in a loop, a context
// runs k_imu_preintegrate, one workgroup of one wavefront per interval -- Jacobian, covariance and the per-sample blocks stay
// in LDS for the whole chain over the samples (13.0 KB, so twelve intervals are resident on a CU) and are written once at the
// end.  One upload (offsets | biases | samples from one pinned block), one launch, one read-back; the input block and the
// output array are MmlStaging pairs, the block laid out by MmlCarve (mml_mem.h), refusals go through mml_refuse.
#include <hip/hip_runtime.h>
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
    imu_preint_interval<false>(samples + 7 * (size_t)s0, cnt, bias + 6 * i, bias + 6 * i + 3, out + i, s_work);
}

}  // namespace

// k_imu_preintegrate on arrays that are on the device already (mml_imu_fetch_batch's packed rows), asynchronous on the
// context's stream; bias: n x (bg | ba).
int mml_launch_imu_preintegrate(mml_ctx* ctx, int n, const double* d_samples, const int* d_offsets, const double* d_bias, mml_imu_preint* d_out) {
    hipLaunchKernelGGL(k_imu_preintegrate, dim3(n), dim3(64), 0, MML_STREAM(ctx), d_samples, d_offsets, d_bias, d_out);
    MML_HIP(hipGetLastError());
    return MML_OK;
}

struct MmlPreintDev {  // each sized for the largest call seen
    MmlStaging<char> in;  // offsets | biases | samples, in bytes
    MmlStaging<mml_imu_preint> out;
    ~MmlPreintDev() {
        in.release();
        out.release();
    }
};

extern "C" int mml_imu_preintegrate_batch(mml_ctx* ctx, int n, const double* samples, const int* offsets, const double* bg,
                                          const double* ba, mml_imu_preint* out) {
    if (n < 1 || n > MML_PREINT_BATCH_MAX) return mml_refuse(ctx, MML_ERR_INVALID, "mml_imu_preintegrate_batch: n = %d is outside 1 .. %d", n, MML_PREINT_BATCH_MAX);
    if (!(offsets && bg && ba && out)) return mml_refuse(ctx, MML_ERR_INVALID, "mml_imu_preintegrate_batch: a null argument");
    if (offsets[0] != 0) return mml_refuse(ctx, MML_ERR_INVALID, "mml_imu_preintegrate_batch: interval 0: offsets[0] is %d, not 0", offsets[0]);
    for (int i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i])
            return mml_refuse(ctx, MML_ERR_INVALID, "mml_imu_preintegrate_batch: interval %d: its end %d lies before its start %d", i, offsets[i + 1], offsets[i]);
    if (!samples && offsets[n] != 0) return mml_refuse(ctx, MML_ERR_INVALID, "mml_imu_preintegrate_batch: samples is null");
    if (!ctx) {  // the host build of the routine
        PreintWork work;
        for (int i = 0; i < n; ++i)
            imu_preint_interval<false>(samples + 7 * (size_t)offsets[i], offsets[i + 1] - offsets[i], bg + 3 * (size_t)i, ba + 3 * (size_t)i, out + i, work);
        return MML_OK;
    }
    MML_HIP(hipSetDevice(ctx->device));
    const size_t total = (size_t)offsets[n];
    MmlCarve<8> c;
    const auto off = c.take<int>((size_t)n + 1);
    const auto bias = c.take<double>(6 * (size_t)n), smp = c.take<double>(7 * total);
    MmlPreintDev* d = mml_side<MmlPreintDev>(ctx, MML_SIDE_PREINT);
    if (d->in.reserve(ctx, c.bytes()) || d->out.reserve(ctx, n)) return MML_ERR_HIP;
    memcpy(off.in(d->in.h), offsets, off.bytes());
    double* h_bias = bias.in(d->in.h);
    for (int i = 0; i < n; ++i) {
        memcpy(h_bias + 6 * (size_t)i, bg + 3 * (size_t)i, sizeof(double) * 3);
        memcpy(h_bias + 6 * (size_t)i + 3, ba + 3 * (size_t)i, sizeof(double) * 3);
    }
    if (total) memcpy(smp.in(d->in.h), samples, smp.bytes());
    hipStream_t s = MML_STREAM(ctx);
    MmlStageScope t(ctx, "imu_preintegrate");
    MML_HIP(hipMemcpyAsync(d->in.d, d->in.h, c.bytes(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_imu_preintegrate, dim3(n), dim3(64), 0, s, smp.in(d->in.d), off.in(d->in.d), bias.in(d->in.d), d->out.d);
    MML_HIP(hipGetLastError());
    MML_HIP(hipMemcpyAsync(d->out.h, d->out.d, sizeof(mml_imu_preint) * n, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    memcpy(out, d->out.h, sizeof(mml_imu_preint) * n);
    return MML_OK;
}
