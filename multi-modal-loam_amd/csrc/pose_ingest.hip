// pose_ingest.hip -- the pose node's way in for a batch of union_cloud messages (unionPoseEstimation.cpp:679-688, :719-773):
//   mml_pose_ingest_plan    the decisions alone, on the host (pose_ingest.h: the rules, with the reference's lines)
//   mml_pose_ingest_batch   the same decisions, then the block of mml_feature_clouds_download_batch into `count` scan slots:
//                           one copy, one table, k_pose_ingest_decode over all frames, k_crop (feature.hip, as it stands) over
//                           the slots, one synchronisation
// k_pose_ingest_decode writes what k_decode_xyzinormal (feature.hip) writes, byte for byte.  That kernel reads twelve floats
// per lane at a 48-byte stride: a wavefront's load instruction touches 64 records = 3 KB for 256 bytes of use, twelve times.
// Here a workgroup takes 256 records of ONE sensor's part of a frame -- a contiguous run of 768 16-byte words --, loads them with
// consecutive lanes on consecutive words (three 1-KB-per-wavefront loads per lane, all in flight together), parks them in LDS
// (12 KB) and reads its own record back.  The compiler narrows those reads to the fields used (two 12-byte reads and a 4-byte
// one).  The record stride of 12 dwords needs no padding for the wide reads: 12 l mod 32 over the eight lanes a 12-byte read
// is served in ({0-3, 20-23} ...) gives eight disjoint 3-bank runs; the one 4-byte read (the intensity) is 4-way conflicted,
// 8 LDS cycles per wavefront against the 3 KB it has just loaded.  The five stores are one point per lane.
// Compiled with -ffp-contract=off like the rest; the one arithmetic operation is the double subtraction of the label test.
#include <string.h>

#include <vector>

#include "mml_internal.h"
#include "pose_ingest.h"

// Table block of mml_pose_ingest_batch (device + pinned twin), grow-only, owned by the context: the call drains the stream
// before it returns, so reserve() never replaces a buffer in use.
struct MmlPoseIngestDev {
    MmlStaging<char> io;
    ~MmlPoseIngestDev() { io.release(); }
};

namespace {

constexpr int PI_TILE = 256;  // records per workgroup = threads per workgroup

struct PoseIngestFrame {  // per frame: where its two parts start in the block (in records) and how many of each are taken
    long long voff, loff;
    int nv, nl;           // nv < 0: a dropped frame, nothing of its slot is touched
    int slot, _pad;
};

struct PoseIngestArrays {
    float4* ln_pts;
    int *ln_gidx, *ln_rel;
    uint8_t *ln_line, *ln_label;
    int *assign_aux, *slot_flags, *cb_n, *fu_info;
    int NV, NT;
};

// grid (tiles, frames, 2 sensors).  words: the block as 16-byte words, three per record.
__global__ __launch_bounds__(PI_TILE) void k_pose_ingest_decode(const float4* __restrict__ words, const PoseIngestFrame* __restrict__ tab,
                                                                PoseIngestArrays A) {
    __shared__ float4 s_rec[3 * PI_TILE];
    const PoseIngestFrame f = tab[blockIdx.y];
    if (f.nv < 0) return;
    const int tid = threadIdx.x, sensor = blockIdx.z, slot = f.slot;
    if (blockIdx.x == 0 && sensor == 0 && tid == 0) {  // what lane 0 of k_decode_xyzinormal leaves for k_crop
        int* a = A.assign_aux + MML_AUX_INTS * (size_t)slot;
        a[MML_AUX_KEPT_VELO] = f.nv;
        a[MML_AUX_KEPT_LIVOX] = f.nl;
        A.slot_flags[2 * slot] = 1;
        A.cb_n[2 * slot] = f.nv;
        A.cb_n[2 * slot + 1] = f.nl;
        int* info = A.fu_info + 8 * (size_t)slot;
        info[4] = 0;
        info[5] = 0;
    }
    const int n = sensor ? f.nl : f.nv;
    const int t0 = blockIdx.x * PI_TILE;
    if (t0 >= n) return;  // (the whole workgroup: no barrier is skipped by a part of it)
    const int m = min(PI_TILE, n - t0);
    const float4* src = words + 3 * ((sensor ? f.loff : f.voff) + t0);
    float4 v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)  // (no branch: a lane past the tile's end loads the last word again; three loads in flight together)
        v[k] = src[min(tid + k * PI_TILE, 3 * m - 1)];
#pragma unroll
    for (int k = 0; k < 3; ++k) s_rec[tid + k * PI_TILE] = v[k];  // (words past 3 m are never read)
    __syncthreads();
    if (tid >= m) return;
    const float4 w0 = s_rec[3 * tid], w1 = s_rec[3 * tid + 1], w2 = s_rec[3 * tid + 2];
    const int i = t0 + tid;  // index inside the sensor's part
    // fused index -> storage position: the Velodyne part from 0, the Livox part from NV
    const size_t o = (size_t)slot * A.NT + (sensor ? A.NV + i : i);
    A.ln_pts[o] = make_float4(w0.x, w0.y, w0.z, w2.x);
    A.ln_gidx[o] = sensor ? f.nv + i : i;
    A.ln_rel[o] = __float_as_int(w1.x);
    const float ln = w1.y, nz = w1.z;
    A.ln_line[o] = (uint8_t)(ln >= 0.f && ln < 255.f ? (int)ln : 255);
    // Estimator.cpp:995-1003: std::abs(normal_z - 1.0) < 1e-5 etc. are evaluated in double on the float field
    uint8_t lab = 0;
    if (fabs((double)nz - 1.0) < 1e-5) lab = 1;
    else if (fabs((double)nz - 2.0) < 1e-5) lab = 2;
    A.ln_label[o] = lab;
}

}  // namespace

extern "C" {

void mml_pose_ingest_opts_default(mml_pose_ingest_opts* opts) {
    if (!opts) return;
    memset(opts, 0, sizeof(*opts));
    opts->hori_rotate_th = 0.3;  // unionPoseEstimation.cpp:147
    opts->velo_rotate_th = 1.5;  // :146
    opts->velo_only_mode = 0;    // :85
    opts->first_frame = -1;
}

int mml_pose_ingest_plan(int count, const int* n_points, const mml_imu_interval* rows, const mml_pose_ingest_opts* opts,
                         mml_pose_ingest_row* out) {
    char msg[192];
    return pose_ingest_plan(count, n_points, rows, opts, out, msg, sizeof(msg));
}

int mml_pose_ingest_batch(mml_ctx* ctx, int first_slot, int count, const uint8_t* clouds, const int* n_points, const mml_imu_interval* rows,
                          const mml_pose_ingest_opts* opts, mml_pose_ingest_row* out) {
    if (!ctx) return MML_ERR_INVALID;
    const char* who = "mml_pose_ingest_batch";
    // ---- every check, before anything is enqueued or written ----
    if (!out) return mml_refuse(ctx, MML_ERR_INVALID, "%s: NULL out", who);
    if (first_slot < 0 || count < 1 || (long)first_slot + count > ctx->B)
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: slots %d .. %ld outside the context's %d (count %d)", who, first_slot,
                          (long)first_slot + count - 1, ctx->B, count);
    char msg[160];
    std::vector<mml_pose_ingest_row> plan((size_t)(count > 0 && count <= MML_POSE_INGEST_MAX ? count : 1));
    int rc = pose_ingest_plan(count, n_points, rows, opts, plan.data(), msg, sizeof(msg));
    if (rc != MML_OK) return mml_refuse(ctx, rc, "%s: %s", who, msg);
    std::vector<PoseIngestFrame> tab((size_t)count);
    long long total = 0;
    int max_part = 0;
    for (int i = 0; i < count; ++i) {
        const int* np = n_points + 6 * i;
        const mml_pose_ingest_row& r = plan[i];
        PoseIngestFrame& f = tab[i];
        f.voff = total + np[0] + np[1];
        f.loff = f.voff + np[2] + np[3] + np[4];
        f.slot = first_slot + i;
        f._pad = 0;
        for (int k = 0; k < 6; ++k) total += np[k];
        if (r.decision == MML_INGEST_DROPPED) {
            f.nv = -1;
            f.nl = 0;
            continue;
        }
        f.nv = r.n_velo;
        f.nl = r.n_points - r.n_velo;
        if (f.nv > ctx->NV)
            return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: frame %d: velo_combine holds %d points, max_velo_points is %d", who, i, f.nv, ctx->NV);
        if (f.nl > ctx->NL)
            return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: frame %d is merged: livox_combine holds %d points, max_livox_points is %d", who, i, f.nl,
                              ctx->NL);
        max_part = f.nv > max_part ? f.nv : max_part;
        max_part = f.nl > max_part ? f.nl : max_part;
    }
    if (total > 0 && !clouds) return mml_refuse(ctx, MML_ERR_INVALID, "%s: NULL clouds with %lld records announced", who, total);
    // ---- the slots: as every entry point that touches a slot range ----
    if (hipSetDevice(ctx->device) != hipSuccess) {
        ctx->err = "hipSetDevice failed";
        return MML_ERR_HIP;
    }
    if (!ctx->uploads.empty()) {
        rc = mml_uploads_wait(ctx, first_slot, count);
        if (rc != MML_OK) return rc;
    }
    hipStream_t s = MML_STREAM(ctx);
    const size_t bytes = (size_t)total * 48, tab_bytes = sizeof(PoseIngestFrame) * (size_t)count;
    rc = ctx->wire_stage.reserve(ctx, bytes ? bytes : 48, s);
    if (rc != MML_OK) return rc;
    MmlPoseIngestDev* d = mml_side<MmlPoseIngestDev>(ctx, MML_SIDE_POSE_INGEST);
    if (d->io.reserve(ctx, tab_bytes, s)) return MML_ERR_HIP;
    // ---- one copy of the block, one table, one decode launch ----
    if (bytes) MML_HIP(hipMemcpyAsync(ctx->wire_stage.d, clouds, bytes, hipMemcpyHostToDevice, s));
    memcpy(d->io.h, tab.data(), tab_bytes);
    MML_HIP(hipMemcpyAsync(d->io.d, d->io.h, tab_bytes, hipMemcpyHostToDevice, s));
    const PoseIngestArrays A{ctx->ln_pts,     ctx->ln_gidx,    ctx->ln_rel, ctx->ln_line, ctx->ln_label, ctx->assign_aux,
                             ctx->slot_flags, ctx->cb_n,       ctx->fu_info, ctx->NV,     ctx->NT};
    const int tiles = max_part > 0 ? (max_part + PI_TILE - 1) / PI_TILE : 1;  // (an empty frame still gets its bookkeeping)
    hipLaunchKernelGGL(k_pose_ingest_decode, dim3(tiles, count, 2), dim3(PI_TILE), 0, s, reinterpret_cast<const float4*>(ctx->wire_stage.d),
                       reinterpret_cast<const PoseIngestFrame*>(d->io.d), A);
    MML_HIP(hipGetLastError());
    // ---- label counts and lists: k_crop over every run of adjacent slots that hold a frame ----
    for (int i = 0; i < count;) {
        if (tab[i].nv < 0) {
            ++i;
            continue;
        }
        int j = i;
        while (j < count && tab[j].nv >= 0) {
            ctx->und_pending[first_slot + j] = 0;  // (the cloud is replaced: nothing of the old one is left to finish)
            ++j;
        }
        rc = mml_launch_cloud_lists(ctx, first_slot + i, j - i);
        if (rc != MML_OK) return rc;
        i = j;
    }
    // the staging buffer is reused by the next wire-format call and the host buffers belong to the caller
    MML_HIP(hipStreamSynchronize(s));
    memcpy(out, plan.data(), sizeof(mml_pose_ingest_row) * (size_t)count);
    return MML_OK;
}

}  // extern "C"
