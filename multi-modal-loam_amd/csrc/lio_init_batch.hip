// lio_init_batch.hip -- mml_lio_initialize_batch: TryMAPInitialization (unionPoseEstimation.cpp:425-625) for n_seg segments in
// one call.  The arithmetic is lio_init_core.h (steps 1-7 of mml_lio_initialize) and imu_preint.h (the pre-integrations before
// and after), one routine each for both sides: a NULL context runs their host builds in a loop over the segments, a context runs
// three launches on its stream --
//   k_lio_preint      a wavefront per frame: the pre-integration frame f holds, at frame f-1's biases (skipped with pre_in)
//   k_lio_initialize  a wavefront per segment, the whole solve state in LDS (LioWork, 50.4 KB: three segments resident on a CU);
//                     writes the segment's state in place and marks the frames of a status-0 segment
//   k_lio_preint      again over the marked frames, reading the new biases from the state the kernel before it wrote
// -- between ONE upload (offsets | times | extrinsics | samples | marks | state, and the given pre-integrations, from one pinned
// block) and ONE read-back (state | results | pre-integrations).  The host applies a segment's bytes unless its status is 3.
// The block is an MmlStaging pair laid out by MmlCarve (mml_mem.h), refusals go through mml_refuse.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "imu_preint.h"
#include "lio_init_core.h"
#include "mml_internal.h"

namespace {

// frame f's pre-integration against frame f - 1, with frame f - 1's biases; go[f] == 0 (a segment's first frame, a segment that
// is not redone) leaves pre[f] alone
__global__ __launch_bounds__(64) void k_lio_preint(const double* samples, const int* sample_offsets, const double* bg, const double* ba,
                                                   const int* go, mml_imu_preint* pre) {
    __shared__ PreintWork s_work;
    const size_t f = blockIdx.x;
    if (!go[f]) return;
    const int s0 = sample_offsets[f], cnt = sample_offsets[f + 1] - s0;
    imu_preint_interval<false>(samples + 7 * (size_t)s0, cnt, bg + 3 * (f - 1), ba + 3 * (f - 1), pre + f, s_work);
}

__global__ __launch_bounds__(64) void k_lio_initialize(const int* frame_offsets, const double* t, double* P, double* Q, double* V, double* bg,
                                                       double* ba, const double* samples, const int* sample_offsets, const double* exTlb,
                                                       const mml_imu_preint* pre, int* go, mml_lio_init_result* out) {
    __shared__ LioWork s_work;
    const int s = blockIdx.x;
    const int f0 = frame_offsets[s], n = frame_offsets[s + 1] - f0;
    const int s0 = sample_offsets[f0], cnt0 = sample_offsets[f0 + 1] - s0;
    const int status = lio_init_segment(n, t + f0, P + 3 * (size_t)f0, Q + 4 * (size_t)f0, V + 3 * (size_t)f0, bg + 3 * (size_t)f0,
                                        ba + 3 * (size_t)f0, samples + 7 * (size_t)s0, cnt0, exTlb + 16 * (size_t)s, pre + f0, out + s, s_work);
    MARG_FOR(i, n) go[f0 + i] = (status == 0 && i >= 1) ? 1 : 0;
}

}  // namespace

struct MmlLioDev {
    MmlStaging<char> blk;  // sized for the largest call seen
    ~MmlLioDev() { blk.release(); }
};

extern "C" int mml_lio_initialize_batch(mml_ctx* ctx, int n_seg, const int* frame_offsets, const double* t, double* P, double* Q, double* V,
                                        double* bg, double* ba, const double* samples, const int* sample_offsets, const double* exTlb,
                                        const mml_imu_preint* pre_in, mml_imu_preint* pre_out, mml_lio_init_result* out) {
    static const char who[] = "mml_lio_initialize_batch";
    if (n_seg < 1 || n_seg > MML_LIO_BATCH_MAX) return mml_refuse(ctx, MML_ERR_INVALID, "%s: n_seg = %d is outside 1 .. %d", who, n_seg, MML_LIO_BATCH_MAX);
    if (!(frame_offsets && t && P && Q && V && bg && ba && samples && sample_offsets && exTlb && out))
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null argument", who);
    if (frame_offsets[0] != 0) return mml_refuse(ctx, MML_ERR_INVALID, "%s: segment 0: frame_offsets[0] is %d, not 0", who, frame_offsets[0]);
    for (int s = 0; s < n_seg; ++s) {
        const long long n = (long long)frame_offsets[s + 1] - frame_offsets[s];
        if (n < 2 || n > MML_LIO_BATCH_MAX_FRAMES)
            return mml_refuse(ctx, MML_ERR_INVALID, "%s: segment %d: %lld frames, outside 2 .. %d", who, s, n, MML_LIO_BATCH_MAX_FRAMES);
    }
    const int F = frame_offsets[n_seg];
    if (sample_offsets[0] != 0) return mml_refuse(ctx, MML_ERR_INVALID, "%s: segment 0: sample_offsets[0] is %d, not 0", who, sample_offsets[0]);
    for (int s = 0; s < n_seg; ++s) {
        const int f0 = frame_offsets[s], f1 = frame_offsets[s + 1];
        for (int f = f0; f < f1; ++f)
            if (sample_offsets[f + 1] < sample_offsets[f])
                return mml_refuse(ctx, MML_ERR_INVALID, "%s: segment %d: frame %d's samples end at %d, before their start %d", who, s, f - f0,
                                  sample_offsets[f + 1], sample_offsets[f]);
        if (sample_offsets[f0 + 1] == sample_offsets[f0])  // GetAverageAcc would divide by zero
            return mml_refuse(ctx, MML_ERR_INVALID, "%s: segment %d: frame 0 has no sample", who, s);
    }
    const size_t total = (size_t)sample_offsets[F];

    if (!ctx) {  // the host build of the two routines
        std::vector<mml_imu_preint> pre(MML_LIO_BATCH_MAX_FRAMES);
        PreintWork* pw = new PreintWork;
        LioWork* lw = new LioWork;
        for (int s = 0; s < n_seg; ++s) {
            const int f0 = frame_offsets[s], n = frame_offsets[s + 1] - f0;
            for (int i = 1; i < n; ++i) {
                const int f = f0 + i;
                if (pre_in)
                    pre[i] = pre_in[f];
                else
                    imu_preint_interval<false>(samples + 7 * (size_t)sample_offsets[f], sample_offsets[f + 1] - sample_offsets[f], bg + 3 * (size_t)(f - 1),
                                        ba + 3 * (size_t)(f - 1), &pre[i], *pw);
            }
            const int status = lio_init_segment(n, t + f0, P + 3 * (size_t)f0, Q + 4 * (size_t)f0, V + 3 * (size_t)f0, bg + 3 * (size_t)f0,
                                                ba + 3 * (size_t)f0, samples + 7 * (size_t)sample_offsets[f0], sample_offsets[f0 + 1] - sample_offsets[f0],
                                                exTlb + 16 * (size_t)s, pre.data(), out + s, *lw);
            if (status == 3) continue;
            if (status == 0)  // frame i pre-integrated again from frame i - 1 with that frame's new biases (:602-609)
                for (int i = 1; i < n; ++i) {
                    const int f = f0 + i;
                    imu_preint_interval<false>(samples + 7 * (size_t)sample_offsets[f], sample_offsets[f + 1] - sample_offsets[f], bg + 3 * (size_t)(f - 1),
                                        ba + 3 * (size_t)(f - 1), &pre[i], *pw);
                }
            if (pre_out)
                for (int i = 1; i < n; ++i) pre_out[f0 + i] = pre[i];
        }
        delete pw;
        delete lw;
        return MML_OK;
    }

    MML_HIP(hipSetDevice(ctx->device));
    // the block: [frame_offsets | sample_offsets | t | exTlb | samples | go] in only, [P | Q | V | bg | ba] both ways,
    // [out | pre] out (pre also in when pre_in is given)
    const size_t nf = (size_t)F, ns = (size_t)n_seg;
    MmlCarve<8> c;
    const auto fo = c.take<int>(ns + 1), so = c.take<int>(nf + 1);
    const auto tt = c.take<double>(nf), ex = c.take<double>(16 * ns), smp = c.take<double>(7 * total);
    const auto go = c.take<int>(nf);
    const auto fP = c.take<double>(3 * nf), fQ = c.take<double>(4 * nf), fV = c.take<double>(3 * nf), fbg = c.take<double>(3 * nf),
               fba = c.take<double>(3 * nf);
    const auto res = c.take<mml_lio_init_result>(ns);
    const auto pre = c.take<mml_imu_preint>(nf);
    const size_t bytes = c.bytes();
    MmlLioDev* d = mml_side<MmlLioDev>(ctx, MML_SIDE_LIO);
    if (d->blk.reserve(ctx, bytes)) return MML_ERR_HIP;
    char* h = d->blk.h;
    char* g = d->blk.d;
    memcpy(fo.in(h), frame_offsets, fo.bytes());
    memcpy(so.in(h), sample_offsets, so.bytes());
    memcpy(tt.in(h), t, tt.bytes());
    memcpy(ex.in(h), exTlb, ex.bytes());
    memcpy(smp.in(h), samples, smp.bytes());
    int* h_go = go.in(h);
    for (int f = 0; f < F; ++f) h_go[f] = 1;
    for (int s = 0; s < n_seg; ++s) h_go[frame_offsets[s]] = 0;
    memcpy(fP.in(h), P, fP.bytes());
    memcpy(fQ.in(h), Q, fQ.bytes());
    memcpy(fV.in(h), V, fV.bytes());
    memcpy(fbg.in(h), bg, fbg.bytes());
    memcpy(fba.in(h), ba, fba.bytes());
    size_t up = res.off;  // everything in front of the results ...
    if (pre_in) {
        memset(h + res.off, 0, pre.off - res.off);
        memcpy(pre.in(h), pre_in, pre.bytes());
        up = bytes;  // ... or the whole block
    }
    hipStream_t st = MML_STREAM(ctx);
    MmlStageScope scope(ctx, "lio_initialize");
    MML_HIP(hipMemcpyAsync(g, h, up, hipMemcpyHostToDevice, st));
    if (!pre_in) {
        hipLaunchKernelGGL(k_lio_preint, dim3(F), dim3(64), 0, st, smp.in(g), so.in(g), fbg.in(g), fba.in(g), go.in(g), pre.in(g));
        MML_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lio_initialize, dim3(n_seg), dim3(64), 0, st, fo.in(g), tt.in(g), fP.in(g), fQ.in(g), fV.in(g), fbg.in(g), fba.in(g),
                       smp.in(g), so.in(g), ex.in(g), pre.in(g), go.in(g), res.in(g));
    MML_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_lio_preint, dim3(F), dim3(64), 0, st, smp.in(g), so.in(g), fbg.in(g), fba.in(g), go.in(g), pre.in(g));
    MML_HIP(hipGetLastError());
    MML_HIP(hipMemcpyAsync(h + fP.off, g + fP.off, bytes - fP.off, hipMemcpyDeviceToHost, st));  // state | results | pre-integrations
    MML_HIP(hipStreamSynchronize(st));
    const mml_lio_init_result* h_out = res.in(h);
    const mml_imu_preint* h_pre = pre.in(h);
    for (int s = 0; s < n_seg; ++s) {
        memcpy(out + s, h_out + s, sizeof(mml_lio_init_result));  // (bytes: the padding too)
        if (h_out[s].status == 3) continue;
        const size_t f0 = (size_t)frame_offsets[s], n = (size_t)frame_offsets[s + 1] - f0;
        memcpy(P + 3 * f0, fP.in(h) + 3 * f0, sizeof(double) * 3 * n);
        memcpy(Q + 4 * f0, fQ.in(h) + 4 * f0, sizeof(double) * 4 * n);
        memcpy(V + 3 * f0, fV.in(h) + 3 * f0, sizeof(double) * 3 * n);
        memcpy(bg + 3 * f0, fbg.in(h) + 3 * f0, sizeof(double) * 3 * n);
        memcpy(ba + 3 * f0, fba.in(h) + 3 * f0, sizeof(double) * 3 * n);
        if (pre_out) memcpy(pre_out + f0 + 1, h_pre + f0 + 1, sizeof(mml_imu_preint) * (n - 1));
    }
    return MML_OK;
}
