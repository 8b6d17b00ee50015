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
// The block is an MmlStaging pair (mml_mem.h), refusals go through mml_refuse.
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
    imu_preint_interval(samples + 7 * (size_t)s0, cnt, bg + 3 * (f - 1), ba + 3 * (f - 1), pre + f, s_work);
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

size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

struct MmlLioDev {
    MmlStaging<char> blk;  // sized for the largest call seen
};

void mml_lio_init_release(mml_ctx* ctx) {
    MmlLioDev* d = ctx->lio;
    if (!d) return;
    d->blk.release();
    delete d;
    ctx->lio = nullptr;
}

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
                    imu_preint_interval(samples + 7 * (size_t)sample_offsets[f], sample_offsets[f + 1] - sample_offsets[f], bg + 3 * (size_t)(f - 1),
                                        ba + 3 * (size_t)(f - 1), &pre[i], *pw);
            }
            const int status = lio_init_segment(n, t + f0, P + 3 * (size_t)f0, Q + 4 * (size_t)f0, V + 3 * (size_t)f0, bg + 3 * (size_t)f0,
                                                ba + 3 * (size_t)f0, samples + 7 * (size_t)sample_offsets[f0], sample_offsets[f0 + 1] - sample_offsets[f0],
                                                exTlb + 16 * (size_t)s, pre.data(), out + s, *lw);
            if (status == 3) continue;
            if (status == 0)  // frame i pre-integrated again from frame i - 1 with that frame's new biases (:602-609)
                for (int i = 1; i < n; ++i) {
                    const int f = f0 + i;
                    imu_preint_interval(samples + 7 * (size_t)sample_offsets[f], sample_offsets[f + 1] - sample_offsets[f], bg + 3 * (size_t)(f - 1),
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
    size_t o = 0;
    const auto take = [&](size_t bytes) {
        const size_t at = o;
        o += align8(bytes);
        return at;
    };
    const size_t o_fo = take(sizeof(int) * ((size_t)n_seg + 1)), o_so = take(sizeof(int) * ((size_t)F + 1)), o_t = take(sizeof(double) * F),
                 o_ex = take(sizeof(double) * 16 * n_seg), o_smp = take(sizeof(double) * 7 * total), o_go = take(sizeof(int) * F),
                 o_P = take(sizeof(double) * 3 * F), o_Q = take(sizeof(double) * 4 * F), o_V = take(sizeof(double) * 3 * F),
                 o_bg = take(sizeof(double) * 3 * F), o_ba = take(sizeof(double) * 3 * F), o_out = take(sizeof(mml_lio_init_result) * n_seg),
                 o_pre = take(sizeof(mml_imu_preint) * F), bytes = o;
    if (!ctx->lio) ctx->lio = new MmlLioDev();
    MmlLioDev* d = ctx->lio;
    if (d->blk.reserve(ctx, bytes)) return MML_ERR_HIP;
    char* h = d->blk.h;
    char* g = d->blk.d;
    memcpy(h + o_fo, frame_offsets, sizeof(int) * ((size_t)n_seg + 1));
    memcpy(h + o_so, sample_offsets, sizeof(int) * ((size_t)F + 1));
    memcpy(h + o_t, t, sizeof(double) * F);
    memcpy(h + o_ex, exTlb, sizeof(double) * 16 * n_seg);
    memcpy(h + o_smp, samples, sizeof(double) * 7 * total);
    int* h_go = reinterpret_cast<int*>(h + o_go);
    for (int f = 0; f < F; ++f) h_go[f] = 1;
    for (int s = 0; s < n_seg; ++s) h_go[frame_offsets[s]] = 0;
    memcpy(h + o_P, P, sizeof(double) * 3 * F);
    memcpy(h + o_Q, Q, sizeof(double) * 4 * F);
    memcpy(h + o_V, V, sizeof(double) * 3 * F);
    memcpy(h + o_bg, bg, sizeof(double) * 3 * F);
    memcpy(h + o_ba, ba, sizeof(double) * 3 * F);
    size_t up = o_out;
    if (pre_in) {
        memset(h + o_out, 0, o_pre - o_out);
        memcpy(h + o_pre, pre_in, sizeof(mml_imu_preint) * F);
        up = bytes;
    }
    hipStream_t st = MML_STREAM(ctx);
    MmlStageScope scope(ctx, "lio_initialize");
    const int* g_so = reinterpret_cast<const int*>(g + o_so);
    const double* g_smp = reinterpret_cast<const double*>(g + o_smp);
    double *g_bg = reinterpret_cast<double*>(g + o_bg), *g_ba = reinterpret_cast<double*>(g + o_ba);
    int* g_go = reinterpret_cast<int*>(g + o_go);
    mml_imu_preint* g_pre = reinterpret_cast<mml_imu_preint*>(g + o_pre);
    MML_HIP(hipMemcpyAsync(g, h, up, hipMemcpyHostToDevice, st));
    if (!pre_in) {
        hipLaunchKernelGGL(k_lio_preint, dim3(F), dim3(64), 0, st, g_smp, g_so, g_bg, g_ba, g_go, g_pre);
        MML_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lio_initialize, dim3(n_seg), dim3(64), 0, st, reinterpret_cast<const int*>(g + o_fo), reinterpret_cast<const double*>(g + o_t),
                       reinterpret_cast<double*>(g + o_P), reinterpret_cast<double*>(g + o_Q), reinterpret_cast<double*>(g + o_V), g_bg, g_ba, g_smp, g_so,
                       reinterpret_cast<const double*>(g + o_ex), g_pre, g_go, reinterpret_cast<mml_lio_init_result*>(g + o_out));
    MML_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_lio_preint, dim3(F), dim3(64), 0, st, g_smp, g_so, g_bg, g_ba, g_go, g_pre);
    MML_HIP(hipGetLastError());
    MML_HIP(hipMemcpyAsync(h + o_P, g + o_P, bytes - o_P, hipMemcpyDeviceToHost, st));
    MML_HIP(hipStreamSynchronize(st));
    const mml_lio_init_result* h_out = reinterpret_cast<const mml_lio_init_result*>(h + o_out);
    const mml_imu_preint* h_pre = reinterpret_cast<const mml_imu_preint*>(h + o_pre);
    for (int s = 0; s < n_seg; ++s) {
        memcpy(out + s, h_out + s, sizeof(mml_lio_init_result));  // (bytes: the padding too)
        if (h_out[s].status == 3) continue;
        const size_t f0 = (size_t)frame_offsets[s], n = (size_t)frame_offsets[s + 1] - f0;
        memcpy(P + 3 * f0, h + o_P + sizeof(double) * 3 * f0, sizeof(double) * 3 * n);
        memcpy(Q + 4 * f0, h + o_Q + sizeof(double) * 4 * f0, sizeof(double) * 4 * n);
        memcpy(V + 3 * f0, h + o_V + sizeof(double) * 3 * f0, sizeof(double) * 3 * n);
        memcpy(bg + 3 * f0, h + o_bg + sizeof(double) * 3 * f0, sizeof(double) * 3 * n);
        memcpy(ba + 3 * f0, h + o_ba + sizeof(double) * 3 * f0, sizeof(double) * 3 * n);
        if (pre_out) memcpy(pre_out + f0 + 1, h_pre + f0 + 1, sizeof(mml_imu_preint) * (n - 1));
    }
    return MML_OK;
}
