// capi.hip -- the C-ABI of libmmloam_hip.so (include/mmloam_hip.h): context, buffers, call sequencing.
// Every entry point validates, stages small parameter blocks through a pinned ring and enqueues the kernels of feature.hip /
// undistort_voxel.hip / map_assoc.hip / solve.hip on the ctx stream.  The only compute that lives here is the kernels of the
// wire decoders, the fused-cloud downloads, the slot digest and the two device probes (copy bandwidth, issue rate).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "imu_math.h"
#include "mml_internal.h"
#include "fused_view_dev.h"
#include "phase_clock.h"
#include "raw_gather_dev.h"
#include "world_map_score.h"

int mml_launch_detect_line(mml_ctx* ctx, int n, uint16_t* d_final);

namespace {

// pinned staging ring for small host<->device parameter blocks
constexpr size_t kStageDoubles = 1u << 22;  // 32 MiB: a 1024-scan step stages ~45 k doubles; a wrap synchronises the device

double* stage_alloc(mml_ctx* ctx, size_t doubles) {
    if (ctx->stage_cursor + doubles > ctx->h_stage_doubles) {
        mml_sync_all(ctx);
        ctx->stage_cursor = 0;
    }
    double* p = ctx->h_stage + ctx->stage_cursor;
    ctx->stage_cursor += (doubles + 7) & ~size_t(7);
    return p;
}

// The launch settings of a context, read once when it is created: the CU count of its device and the environment switches.
// Nothing else in the library reads the environment, so every choice below holds for this context alone.
hipError_t read_settings(mml_ctx* ctx) {
    hipDeviceProp_t prop;
    const hipError_t e = hipGetDeviceProperties(&prop, ctx->device);
    if (e != hipSuccess) return e;
    ctx->cus = prop.multiProcessorCount;
    // (two lanes: with calls of ~2000 scans two to four lanes give the same rate, with 8192 two give 360 k scans/s against 351 k for
    //  four, and a call of a few hundred scans splits into launches that still fill the device)
    ctx->n_lanes = 2;
    if (const char* v = getenv("MML_LANES")) {  // tuning knob: number of stream lanes mml_step pipelines over
        const int n = atoi(v);
        if (n >= 1 && n <= mml_ctx::MAX_LANES) ctx->n_lanes = n;
    }
    // measurement switches, each selecting the other form of a stage (same results bit for bit)
    const auto off = [](const char* name) {
        const char* v = getenv(name);
        return v && atoi(v) == 0;
    };
    ctx->onepass_wanted = !off("MML_ASSIGN_ONEPASS");
    ctx->solve_wide = !off("MML_SOLVE_WIDE");
    ctx->use_graph = getenv("MML_NO_GRAPH") == nullptr;
    ctx->lazy_undistort = !off("MML_LAZY_UNDISTORT");
    return hipSuccess;
}

}  // namespace

double* mml_stage_alloc(mml_ctx* ctx, size_t doubles) { return stage_alloc(ctx, doubles); }

int mml_refuse(mml_ctx* ctx, int code, const char* fmt, ...) {
    if (ctx) {  // (a NULL context has nowhere to carry the message)
        char m[192];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(m, sizeof(m), fmt, ap);
        va_end(ap);
        ctx->err = m;
    }
    return code;
}

extern "C" {

void mml_config_default(mml_config* cfg, int max_scans) {
    memset(cfg, 0, sizeof(*cfg));
    cfg->max_scans = max_scans;
    cfg->max_velo_points = 16 * 1800;
    cfg->max_livox_points = 24000;
    cfg->n_rings = 16;
    cfg->pitch0_deg = -15.0f;
    cfg->pitch_step_deg = 2.0f;
    cfg->n_livox_lines = 6;
    cfg->near_th = 2.0f;
    cfg->far_th = 50.0f;
    cfg->leaf_corner = 0.4f;
    cfg->leaf_surf = 0.2f;
    cfg->cell_corner = 0.f;
    cfg->cell_surf = 0.f;
    cfg->max_features = 0;
    cfg->max_map_points = 0;
}

int mml_abi_version(void) { return MML_ABI_VERSION; }

const char* mml_last_error(const mml_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int mml_config_get(const mml_ctx* ctx, mml_config* out) {
    if (!ctx || !out) return MML_ERR_INVALID;
    *out = ctx->cfg;
    return MML_OK;
}

void mml_destroy(mml_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    for (int l = 0; l < mml_ctx::MAX_LANES; ++l)
        if (ctx->streams[l]) hipStreamSynchronize(ctx->streams[l]);
    if (ctx->copy_stream) hipStreamSynchronize(ctx->copy_stream);
    mml_comm_destroy(ctx);
    ctx->side.release();
    ctx->release_memory();
    for (auto& pe : ctx->pending) {
        hipEventDestroy(pe.a);
        hipEventDestroy(pe.b);
    }
    for (auto e : ctx->event_pool) hipEventDestroy(e);
    for (auto& g : ctx->win_graphs) hipGraphExecDestroy(g.exec);
    for (auto& u : ctx->uploads) hipEventDestroy(u.done);
    for (auto e : ctx->upload_event_pool) hipEventDestroy(e);
    for (int l = 0; l < mml_ctx::MAX_LANES; ++l) {
        if (ctx->lane_mark[l]) hipEventDestroy(ctx->lane_mark[l]);
        if (ctx->streams[l]) hipStreamDestroy(ctx->streams[l]);
    }
    if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
    delete ctx;
}

int mml_create(const mml_config* cfg, int device, mml_ctx** out) {
    if (!cfg || !out) return MML_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MML_ERR_NO_DEVICE;  // no CPU fallback
    if (device < 0 || device >= ndev) return MML_ERR_NO_DEVICE;
    if (cfg->max_scans <= 0 || cfg->max_velo_points < 0 || cfg->max_livox_points < 0 || cfg->n_rings <= 0 ||
        cfg->n_rings > 128 || cfg->n_livox_lines <= 0 || cfg->n_livox_lines > 32)
        return MML_ERR_INVALID;
    mml_ctx* ctx = new mml_ctx();
    ctx->cfg = *cfg;
    ctx->device = device;
    if (ctx->cfg.cell_corner <= 0) ctx->cfg.cell_corner = 5.0f * ctx->cfg.leaf_corner;
    if (ctx->cfg.cell_surf <= 0) ctx->cfg.cell_surf = 5.0f * ctx->cfg.leaf_surf;
    if (ctx->cfg.max_features <= 0) ctx->cfg.max_features = 8192;
    if (ctx->cfg.max_map_points <= 0) ctx->cfg.max_map_points = 1 << 21;
    ctx->B = cfg->max_scans;
    ctx->NV = (cfg->max_velo_points + 63) & ~63;
    ctx->NL = (cfg->max_livox_points + 63) & ~63;
    ctx->NT = ctx->NV + ctx->NL;
    ctx->L = cfg->n_rings + cfg->n_livox_lines;
    ctx->MF = ctx->cfg.max_features;
    ctx->MM = ctx->cfg.max_map_points;
    // label lists per (slot, kind) hold every labelled point (8 B x NT per slot): up to MML_VOXEL_LDS_CAP of them feed
    // the LDS sort of k_voxel, denser labelled clouds and scans beyond 64k points (e.g. 128 x 2048 rings) take the
    // global-sort filter (mml_downsample_big)
    ctx->VX_CAP = (int)ctx->NT;
    ctx->h_n_in.assign((size_t)ctx->B * 2, 0);
    ctx->raw_extracted.assign((size_t)ctx->B, 0);
    ctx->stats_stale.assign((size_t)ctx->B, 1);
    ctx->und_pending.assign((size_t)ctx->B, 0);
    auto fail = [&](hipError_t e, const char* what) {
        ctx->err = std::string(what) + ": " + hipGetErrorString(e);
        // keep ctx alive so the caller can read the message? No: report through the return code only.
        mml_destroy(ctx);
        return MML_ERR_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail(e, "hipSetDevice");
    if ((e = read_settings(ctx)) != hipSuccess) return fail(e, "hipGetDeviceProperties");
    for (int l = 0; l < mml_ctx::MAX_LANES; ++l) {
        if ((e = hipStreamCreateWithFlags(&ctx->streams[l], hipStreamNonBlocking)) != hipSuccess)
            return fail(e, "hipStreamCreate");
        if ((e = hipEventCreateWithFlags(&ctx->lane_mark[l], hipEventDisableTiming)) != hipSuccess)
            return fail(e, "hipEventCreate");
    }
    if ((e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
    const size_t B = ctx->B, NV = ctx->NV, NL = ctx->NL, NT = ctx->NT, L = ctx->L, MF = ctx->MF, MM = ctx->MM;
#define ALLOC(ptr, n)                                                  \
    if ((e = ctx->fixed.alloc(&(ptr), (n))) != hipSuccess) return fail(e, #ptr); \
    if ((e = hipMemsetAsync((ptr), 0, sizeof(*(ptr)) * ((n) ? (n) : 1), MML_STREAM(ctx))) != hipSuccess) return fail(e, #ptr)
    ALLOC(ctx->velo_in, B * NV);
    ALLOC(ctx->livox_in, B * NL);
    ALLOC(ctx->d_n_in, B * 2);
    ALLOC(ctx->raw_line, B * NT);
    ALLOC(ctx->raw_ori, B * NV);
    ALLOC(ctx->ln_pts, B * NT);
    ALLOC(ctx->ln_gidx, B * NT);
    ALLOC(ctx->ln_rel, B * NT);
    ALLOC(ctx->slot_flags, B * 2);
    ALLOC(ctx->line_start, B * L);
    ALLOC(ctx->line_len, B * L);
    ALLOC(ctx->seg_cum, B * L * (MML_SEG_MAX + 1));
    ALLOC(ctx->seg_pos, B * L * MML_SEG_MAX);
    ALLOC(ctx->seg_n, B * L);
    ALLOC(ctx->seg_flat, B * 2 * MML_SEG_FLAT);
    ALLOC(ctx->seg_flat_n, B * 4);
    ALLOC(ctx->op_agg, B * 2 * MML_SEG_MAX);
    ctx->seg_rstride = (int)((NT >> 6) + 6 * L + 8);
    ALLOC(ctx->seg_rs, B * (size_t)ctx->seg_rstride);
    ALLOC(ctx->seg_rw, B * (size_t)ctx->seg_rstride);
    ALLOC(ctx->ln_curv, B * NT);
    ALLOC(ctx->ln_refl, B * NT);
    ALLOC(ctx->ln_attr, B * NT);
    ALLOC(ctx->sel_scratch, 4 * B * NT + 16 * B * (L + 2) + 64);
    {
        const size_t nblk = ((NV > NL ? NV : NL) + 255) / 256;
        ALLOC(ctx->blk_cnt, B * 2 * nblk * 162);
    }
    ALLOC(ctx->assign_aux, B * 8);
    ALLOC(ctx->brk_queue, B * NT);
    ALLOC(ctx->brk_cnt, 2 * B);
    ALLOC(ctx->queue_off, 2 * ((size_t)B + mml_ctx::MAX_LANES + 1));
    ALLOC(ctx->redo_queue, B * NT);
    ALLOC(ctx->st_exit, B * (NT / 256 + L + 8));
    ALLOC(ctx->vx_big, 2 * B);
    ALLOC(ctx->sel_done, B * L + 8);
    ALLOC(ctx->sel_list, 4 * B * L + 8);
    ALLOC(ctx->sel_list_cnt, 2 * B + 8);
    ALLOC(ctx->crop_cnt, B * ((NT + 255) / 256) * 8);
    ALLOC(ctx->cb_n, B * 2);
    ALLOC(ctx->ln_line, B * NT);
    ALLOC(ctx->ln_label, B * NT);
    ALLOC(ctx->fu_info, B * 8);
    ALLOC(ctx->ft_xyz[0], B * MF);
    ALLOC(ctx->ft_xyz[1], B * MF);
    ALLOC(ctx->ft_n, B * 2);
    ALLOC(ctx->vx_keys, B * (size_t)ctx->VX_CAP);  // B*2*VX_CAP unsigned
    ALLOC(ctx->vx_gidx, 2 * B * (size_t)ctx->VX_CAP);
    ALLOC(ctx->lf, B * MF);
    ALLOC(ctx->pf, B * MF);
    ALLOC(ctx->assoc_stats, B * 16);
    ALLOC(ctx->hard_list, B * MF * 2);
    ALLOC(ctx->hard_knn, B * MF * 2 * 10);
    ALLOC(ctx->work_off, 2 * B + 8);
    if (mml_map_local_alloc(ctx, ctx->own) != MML_OK) return fail(hipErrorOutOfMemory, "the own local map");
    ALLOC(ctx->map_keys, MM);
    ALLOC(ctx->map_keys2, MM);
    ALLOC(ctx->map_vals, MM);
    ALLOC(ctx->map_vals2, MM);
    ALLOC(ctx->d_x, B * 6);
    ALLOC(ctx->d_pose_in, B * kPoseSlotDoubles);
    ALLOC(ctx->d_result, B * MML_SOLVE_RESULT);
    ALLOC(ctx->d_summ, B * 8);
    ALLOC(ctx->d_trace, B * 6 * 64);
    ALLOC(ctx->d_rec, B * 32);
    ALLOC(ctx->d_und, B * 8);
    ALLOC(ctx->d_und_par, B * 12);
    ALLOC(ctx->d_extr, 16);
    ALLOC(ctx->d_misc, 64);
#undef ALLOC
    ctx->h_stage_doubles = kStageDoubles;
    if ((e = ctx->fixed.alloc_pinned(&ctx->h_stage, ctx->h_stage_doubles + 8)) != hipSuccess) return fail(e, "ctx->h_stage");
    ctx->stage_cursor = 0;
    if (mml_feature_init(ctx) != MML_OK) return fail(hipErrorUnknown, "mml_feature_init");
    if ((e = hipStreamSynchronize(MML_STREAM(ctx))) != hipSuccess) return fail(e, "hipStreamSynchronize");
    *out = ctx;
    return MML_OK;
}

int mml_synchronize(mml_ctx* ctx) {
    if (!ctx) return MML_ERR_INVALID;
    return mml_sync_all(ctx);
}

static int check_slots(mml_ctx* ctx, int first, int count) {
    MML_REQUIRE(ctx != nullptr, MML_ERR_INVALID, "null ctx");
    MML_REQUIRE(first >= 0 && count > 0 && first + count <= ctx->B, MML_ERR_INVALID, "slot range out of bounds");
    return MML_OK;
}
#define CHECK_SLOTS(first, count)                        \
    do {                                                 \
        if (!ctx) return MML_ERR_INVALID;                \
        int rc_ = check_slots(ctx, (first), (count));    \
        if (rc_ != MML_OK) return rc_;                   \
        if (hipSetDevice(ctx->device) != hipSuccess) {   \
            ctx->err = "hipSetDevice failed";            \
            return MML_ERR_HIP;                          \
        }                                                \
        if (!ctx->uploads.empty()) {                     \
            rc_ = mml_uploads_wait(ctx, (first), (count)); \
            if (rc_ != MML_OK) return rc_;               \
        }                                                \
    } while (0)

// copy a block of doubles to the device through the pinned ring (asynchronous, safe against reuse)
static int upload_doubles(mml_ctx* ctx, double* d_dst, const double* h_src, size_t n) {
    double* st = stage_alloc(ctx, n);
    memcpy(st, h_src, sizeof(double) * n);
    MML_HIP(hipMemcpyAsync(d_dst, st, sizeof(double) * n, hipMemcpyHostToDevice, MML_STREAM(ctx)));
    return MML_OK;
}

int mml_scan_upload(mml_ctx* ctx, int slot, const float* velo_xyzi, int n_velo, const mml_livox_point* livox,
                    int n_livox) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE(n_velo >= 0 && n_livox >= 0, MML_ERR_INVALID, "negative point count");
    MML_REQUIRE(n_velo <= ctx->cfg.max_velo_points && n_livox <= ctx->cfg.max_livox_points, MML_ERR_CAPACITY,
                "scan exceeds max_velo_points / max_livox_points");
    MML_REQUIRE((n_velo == 0 || velo_xyzi) && (n_livox == 0 || livox), MML_ERR_INVALID, "null point buffer");
    if (n_velo)
        MML_HIP(hipMemcpyAsync(ctx->velo_in + (size_t)slot * ctx->NV, velo_xyzi, sizeof(float) * 4 * (size_t)n_velo,
                               hipMemcpyHostToDevice, MML_STREAM(ctx)));
    if (n_livox)
        MML_HIP(hipMemcpyAsync(ctx->livox_in + (size_t)slot * ctx->NL, livox, sizeof(mml_livox_point) * (size_t)n_livox,
                               hipMemcpyHostToDevice, MML_STREAM(ctx)));
    ctx->h_n_in[2 * slot] = n_velo;
    ctx->raw_extracted[slot] = 0;
    ctx->h_n_in[2 * slot + 1] = n_livox;
    // counts travel through the pinned ring as raw bytes
    double* st = stage_alloc(ctx, 1);
    int* sti = reinterpret_cast<int*>(st);
    sti[0] = n_velo;
    sti[1] = n_livox;
    MML_HIP(hipMemcpyAsync(ctx->d_n_in + 2 * slot, sti, sizeof(int) * 2, hipMemcpyHostToDevice, MML_STREAM(ctx)));
    return MML_OK;
}

int mml_scan_upload_batch(mml_ctx* ctx, int first_slot, int count, const float* velo_base, const int* n_velo,
                          const mml_livox_point* livox_base, const int* n_livox) {
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(n_velo && n_livox, MML_ERR_INVALID, "null count arrays");
    MML_REQUIRE(ctx->NV == ctx->cfg.max_velo_points && ctx->NL == ctx->cfg.max_livox_points, MML_ERR_INVALID,
                "mml_scan_upload_batch needs max_velo_points / max_livox_points that are multiples of 64 (the slot stride)");
    bool any_v = false, any_l = false;
    for (int i = 0; i < count; ++i) {
        MML_REQUIRE(n_velo[i] >= 0 && n_livox[i] >= 0, MML_ERR_INVALID, "negative point count");
        MML_REQUIRE(n_velo[i] <= ctx->cfg.max_velo_points && n_livox[i] <= ctx->cfg.max_livox_points, MML_ERR_CAPACITY,
                    "scan exceeds max_velo_points / max_livox_points");
        any_v = any_v || n_velo[i] > 0;
        any_l = any_l || n_livox[i] > 0;
    }
    MML_REQUIRE((!any_v || velo_base) && (!any_l || livox_base), MML_ERR_INVALID, "null point buffer");
    // the copies go behind everything already enqueued on the lanes (a kernel may still be reading these slots) ...
    hipStream_t cs = ctx->copy_stream;
    for (int l = 0; l < mml_ctx::MAX_LANES; ++l) {
        MML_HIP(hipEventRecord(ctx->lane_mark[l], ctx->streams[l]));
        MML_HIP(hipStreamWaitEvent(cs, ctx->lane_mark[l], 0));
    }
    if (any_v)
        MML_HIP(hipMemcpyAsync(ctx->velo_in + (size_t)first_slot * ctx->NV, velo_base, sizeof(float4) * (size_t)count * ctx->NV,
                               hipMemcpyHostToDevice, cs));
    if (any_l)
        MML_HIP(hipMemcpyAsync(ctx->livox_in + (size_t)first_slot * ctx->NL, livox_base, sizeof(mml_livox_point) * (size_t)count * ctx->NL,
                               hipMemcpyHostToDevice, cs));
    double* st = stage_alloc(ctx, (size_t)count);
    int* sti = reinterpret_cast<int*>(st);
    for (int i = 0; i < count; ++i) {
        ctx->h_n_in[2 * (first_slot + i)] = sti[2 * i] = n_velo[i];
        ctx->raw_extracted[first_slot + i] = 0;
        ctx->h_n_in[2 * (first_slot + i) + 1] = sti[2 * i + 1] = n_livox[i];
    }
    MML_HIP(hipMemcpyAsync(ctx->d_n_in + 2 * (size_t)first_slot, sti, sizeof(int) * 2 * (size_t)count, hipMemcpyHostToDevice, cs));
    // ... and whatever touches these slots next waits for them (CHECK_SLOTS -> mml_uploads_wait); work on other slots
    // enqueued from now on runs concurrently with the copy
    mml_ctx::Upload u;
    u.first = first_slot;
    u.count = count;
    if (!ctx->upload_event_pool.empty()) {
        u.done = ctx->upload_event_pool.back();
        ctx->upload_event_pool.pop_back();
    } else {
        MML_HIP(hipEventCreateWithFlags(&u.done, hipEventDisableTiming));
    }
    MML_HIP(hipEventRecord(u.done, cs));
    ctx->uploads.push_back(u);
    return MML_OK;
}

// The aligner's frame assembly (livox_stream.hip).  Every refusal for an argument comes before the slots are touched.
int mml_union_assemble(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count, const uint64_t* stamps, const float* velo_xyzi,
                       const int* velo_offsets, const float* tf, mml_union_frame* out) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = mml_union_check(ctx, s, first_slot, count, stamps, velo_xyzi, velo_offsets, out);
    if (rc != MML_OK) return rc;
    CHECK_SLOTS(first_slot, count);
    return mml_union_run(ctx, s, first_slot, count, stamps, velo_xyzi, velo_offsets, tf, out);
}

int mml_union_assemble_offset(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count, const uint64_t* starts, int sliced_points,
                              const float* velo_xyzi, const int* velo_offsets, const float* tf, mml_union_frame* out) {
    if (!ctx) return MML_ERR_INVALID;
    const int rc = mml_union_offset_check(ctx, s, first_slot, count, starts, sliced_points, velo_xyzi, velo_offsets, out);
    if (rc != MML_OK) return rc;
    CHECK_SLOTS(first_slot, count);
    return mml_union_offset_run(ctx, s, first_slot, count, starts, sliced_points, velo_xyzi, velo_offsets, tf, out);
}

int mml_scan_raw_download(mml_ctx* ctx, int slot, float* velo_xyzi, int cap_velo, mml_livox_point* livox, int cap_livox, int* n_velo,
                          int* n_livox) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE(n_velo && n_livox, MML_ERR_INVALID, "null count outputs");
    const int nv = ctx->h_n_in[2 * slot], nl = ctx->h_n_in[2 * slot + 1];
    *n_velo = nv;
    *n_livox = nl;
    MML_REQUIRE((!velo_xyzi || cap_velo >= nv) && (!livox || cap_livox >= nl), MML_ERR_CAPACITY, "download capacity too small");
    if (velo_xyzi && nv)
        MML_HIP(hipMemcpyAsync(velo_xyzi, ctx->velo_in + (size_t)slot * ctx->NV, sizeof(float4) * (size_t)nv, hipMemcpyDeviceToHost,
                               MML_STREAM(ctx)));
    if (livox && nl)
        MML_HIP(hipMemcpyAsync(livox, ctx->livox_in + (size_t)slot * ctx->NL, sizeof(mml_livox_point) * (size_t)nl, hipMemcpyDeviceToHost,
                               MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    return MML_OK;
}

// ---- wire formats ---------------------------------------------------------------------
namespace {
__device__ __forceinline__ float load_f32_unaligned(const uint8_t* p) {
    const unsigned u = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
    return __uint_as_float(u);
}
// pcl::fromROSMsg<PointXYZI> on the device: fields located by byte offset inside point_step-sized records
__global__ void k_decode_pointcloud2(const uint8_t* raw, int n, int step, int ox, int oy, int oz, int oi, float4* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = raw + (size_t)i * step;
    float4 v;
    v.x = load_f32_unaligned(p + ox);
    v.y = load_f32_unaligned(p + oy);
    v.z = load_f32_unaligned(p + oz);
    v.w = oi >= 0 ? load_f32_unaligned(p + oi) : 0.f;
    out[i] = v;
}
// serialised livox_ros_driver/CustomPoint records (19 bytes, unaligned) -> the 20-byte structs of livox_in
__global__ void k_decode_custompoints(const uint8_t* raw, int n, mml_livox_point* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = raw + (size_t)i * 19;
    mml_livox_point q;
    q.offset_time = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    q.x = load_f32_unaligned(p + 4);
    q.y = load_f32_unaligned(p + 8);
    q.z = load_f32_unaligned(p + 12);
    q.reflectivity = p[16];
    q.tag = p[17];
    q.line = p[18];
    q._pad = 0;
    out[i] = q;
}
// (FusedView / fused_at, the fused cloud [velo_combine ; livox_combine] in its own order: fused_view_dev.h)
// pcl::toROSMsg<PointXYZINormal> payload: 48-byte records, x y z 1 | normal_x normal_y normal_z 0 | intensity curvature 0 0
__global__ void k_encode_xyzinormal(FusedView V, float* out) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    int g, line;
    float4 p;
    float rel;
    if (!fused_at(V, pos, g, p, rel, line)) return;
    float* o = out + 12 * (size_t)g;
    o[0] = p.x;
    o[1] = p.y;
    o[2] = p.z;
    o[3] = 1.0f;
    o[4] = rel;                    // normal_x: in-sweep time (unionFeatureExtract.cpp:1186)
    o[5] = (float)line;            // normal_y: ring / Livox line
    o[6] = (float)V.label[pos];    // normal_z: 0 none, 1 corner, 2 surf (:1018-1021)
    o[7] = 0.f;
    o[8] = p.w;                    // intensity
    o[9] = 0.f;                    // curvature
    o[10] = 0.f;
    o[11] = 0.f;
}
// the same record as three 16-byte stores (the batched feature-cloud download)
__device__ __forceinline__ void put_xyzinormal(float4* o, float x, float y, float z, float rel, float line, float label, float intensity) {
    o[0] = make_float4(x, y, z, 1.0f);
    o[1] = make_float4(rel, line, label, 0.f);
    o[2] = make_float4(intensity, 0.f, 0.f, 0.f);
}
// the same cloud as four arrays (mml_scan_download): xyzi | reltime | line | label, back to back in one staging buffer
__global__ void k_fused_arrays(FusedView V, int n, float4* xyzi, float* rel, uint8_t* line, uint8_t* label) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    int g, ln;
    float4 p;
    float r;
    if (!fused_at(V, pos, g, p, r, ln)) return;
    xyzi[g] = p;
    rel[g] = r;
    line[g] = (uint8_t)ln;
    label[g] = V.label[pos];
}
// (SlotArrays / slot_view, the view of one slot derived on the device from the context-wide arrays: fused_view_dev.h)
// The registered cloud (unionPoseEstimation.cpp:896-903): every fused point of slot A.first + blockIdx.y through
// pointAssociateToMap (:199-213) with that slot's pose, as the PointXYZINormal the loop pushes back -- a default-constructed
// point (x y z 1 | 0 0 0 0 | 0 0 0 0) that receives x y z, intensity and normal_z only.  pout = R * pin + t in double, in Eigen's
// order (R0 x + R1 y) + R2 z, then + t, no contraction (-ffp-contract=off), rounded once to float.  par: the call's poses
// (16 doubles each, row-major), then its record offsets (one long long each); lane `pos` writes record rec_off[slot] + g as
// three 16-byte stores.
__global__ void __launch_bounds__(256) k_encode_registered(SlotArrays A, const double* par, int count, float4* out) {
    const int i = blockIdx.y, slot = A.first + i;
    const FusedView V = slot_view(A, slot);
    const int b0 = blockIdx.x * blockDim.x, cv = V.cb_n[0], cl = V.cb_n[1];
    // nothing of this block is a valid position: it lies in the unused tail of the Velodyne region or past the Livox part
    if (b0 >= V.NV + cl || (b0 >= cv && b0 + (int)blockDim.x <= V.NV)) return;
    int g, line;
    float4 p;
    float rel;
    if (!fused_at(V, b0 + threadIdx.x, g, p, rel, line)) return;
    if (g >= A.fu_info[8 * (size_t)slot]) return;  // (the records of the slot end at its count, whatever the index array holds)
    const double* T = par + 16 * (size_t)i;
    const long long rec_off = reinterpret_cast<const long long*>(par + 16 * (size_t)count)[i];
    const double x = p.x, y = p.y, z = p.z;
    float4 a, b, c;
    mml_world_point(T, x, y, z, a.x, a.y, a.z);  // (world_map_key.h: the one definition, shared with the world map)
    a.w = 1.0f;
    b.x = 0.f;
    b.y = 0.f;
    b.z = (float)V.label[b0 + threadIdx.x];  // normal_z: the label (:212)
    b.w = 0.f;
    c.x = p.w;                               // intensity (:211)
    c.y = 0.f;
    c.z = 0.f;
    c.w = 0.f;
    float4* o = out + 3 * (size_t)(rec_off + g);
    o[0] = a;
    o[1] = b;
    o[2] = c;
}
// ---- mml_feature_clouds_download_batch: the six clouds of union_cloud.msg:4-9 per slot ------------------------------------------
// off: where cloud (i, k) starts in `out`, in records -- 6 entries per slot of the call in message order (k: 0 velo_corner,
// 1 velo_surface, 2 velo_combine, 3 livox_corner, 4 livox_surface, 5 livox_combine) and the call's total behind them, so cloud
// (i, k) has room for off[6 i + k + 1] - off[6 i + k] records.
//
// k = 2, 5: the records of k_encode_xyzinormal, the fused index split at the Velodyne count.  grid (blocks of NT, slots)
__global__ void __launch_bounds__(256) k_encode_combine(SlotArrays A, const long long* off, float4* out) {
    const int i = blockIdx.y, slot = A.first + i;
    const FusedView V = slot_view(A, slot);
    const int b0 = blockIdx.x * blockDim.x, cv = V.cb_n[0], cl = V.cb_n[1];
    if (b0 >= V.NV + cl || (b0 >= cv && b0 + (int)blockDim.x <= V.NV)) return;  // (as k_encode_registered)
    int g, line;
    float4 p;
    float rel;
    if (!fused_at(V, b0 + threadIdx.x, g, p, rel, line)) return;
    const int n = A.fu_info[8 * (size_t)slot], nv = A.fu_info[8 * (size_t)slot + 1];
    if (g >= n) return;  // (the records of the slot end at its count, whatever the index array holds)
    const long long at = g < nv ? off[6 * (size_t)i + 2] + g : off[6 * (size_t)i + 5] + (g - nv);
    put_xyzinormal(out + 3 * (size_t)at, p.x, p.y, p.z, rel, (float)line, (float)V.label[b0 + threadIdx.x], p.w);
}
// k = 0, 1, 3, 4: the labelled points of a sensor in the order of its RAW cloud, as getVeloFeature copies them out before it
// zeroes the intensity (unionFeatureExtract.cpp:1244-1252; cropped near + far, :1287-1295) and getHoriFeatureExtract before
// anything is transformed (:1025-1032; cropped near only, :925 / :933 -- the label bytes 0x81 / 0x82 are its points beyond far_th).
// Coordinates and intensity are the raw record's: ln_pts holds the Livox part under the extrinsic once one was applied, and the
// reference transforms livox_combine alone (:312).  In-sweep time and label come from the point's bucketed position
// (raw_gather_dev.h).  grid (2 sensors, slots); a record goes out only where the table has room for it, and got[6 i + k] is
// what the walk found, which the host holds against the counters the table was laid out from.
struct FeatCloudArgs {
    const uint8_t* raw_line;
    const int *n_in, *seg_flat, *seg_flat_n;
    const uint8_t* label;
    const int* rel;
    const float4* velo_in;
    const mml_livox_point* livox_in;
    int first, NT, NV, NL, blk_points;
};
__global__ __launch_bounds__(RG_THREADS) void k_feature_gather(FeatCloudArgs A, const long long* off, float4* out, int* got) {
    const int sensor = blockIdx.x, i = blockIdx.y, slot = A.first + i;
    const size_t o = (size_t)slot * A.NT;
    const uint8_t* label = A.label + o;
    const int* rel = A.rel + o;
    const float4* velo = A.velo_in + (size_t)slot * A.NV;
    const mml_livox_point* livox = A.livox_in + (size_t)slot * A.NL;
    const long long* my_off = off + 6 * (size_t)i + 3 * sensor;
    const long long at0 = my_off[0], at1 = my_off[1], end1 = my_off[2];
    const RawGatherSrc S{A.raw_line + o + (sensor == 0 ? 0 : A.NV), A.seg_flat + ((size_t)slot * 2 + sensor) * MML_SEG_FLAT,
                         A.n_in[2 * (size_t)slot + sensor], A.seg_flat_n[(size_t)slot * 4 + 2 * sensor + 1], A.blk_points, MML_SEG_FLAT, A.NT};
    const unsigned lim = sensor == 0 ? 0x80u : 0x100u;
    int n_out[2];
    raw_gather_walk(
        S,
        [&](int p) {
            const unsigned l = label[p];
            return ((l & 3u) == 1u || (l & 3u) == 2u) && l < lim ? (int)(l & 3u) - 1 : -1;
        },
        [&](int c, int at, int r, int p, int key) {
            if (at >= (int)(c ? end1 - at1 : at1 - at0)) return;
            float4 q;
            if (sensor == 0) {
                q = velo[r];
            } else {
                const mml_livox_point v = livox[r];
                q = make_float4(v.x, v.y, v.z, (float)v.reflectivity);
            }
            put_xyzinormal(out + 3 * (size_t)((c ? at1 : at0) + at), q.x, q.y, q.z, __int_as_float(rel[p]), (float)key, (float)(c + 1), q.w);
        },
        n_out);
    if (threadIdx.x < 2) got[6 * (size_t)i + 3 * sensor + threadIdx.x] = threadIdx.x ? n_out[1] : n_out[0];
}
// ---- mml_slot_digest: order-independent 64-bit digests of what the download entry points would hand out -----------------------
__host__ __device__ __forceinline__ unsigned long long dg_mix(unsigned long long z) {  // splitmix64 finaliser
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ULL;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return z;
}
__host__ __device__ __forceinline__ unsigned long long dg_key(unsigned long long i, unsigned tag) {
    return dg_mix(i * 0x9E3779B97F4A7C15ULL + tag);
}
__device__ __forceinline__ unsigned long long dg_pair(float a, float b) {
    return (unsigned long long)__float_as_uint(a) | ((unsigned long long)__float_as_uint(b) << 32);
}
__device__ __forceinline__ unsigned long long dg_dbits(double d) { return (unsigned long long)__double_as_longlong(d); }
// sum over the workgroup, one atomic per wavefront
__device__ __forceinline__ void dg_commit(unsigned long long v, unsigned long long* dst) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = (unsigned long long)__shfl_down(lo, o) | ((unsigned long long)__shfl_down(hi, o) << 32);
        v += t;
        lo = (unsigned)v;
        hi = (unsigned)(v >> 32);
    }
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}
struct DigestArgs : SlotArrays {
    const int* ft_n;
    const float4* ft[2];
    const MmlLineFactor* lf;
    const MmlPlaneFactor* pf;
    const double* x;
    int B, MF;
};
// pieces 1-4: the fused cloud, one storage position per thread (blockIdx.y = slot of the call)
__global__ void __launch_bounds__(256) k_digest_cloud(DigestArgs A, unsigned long long* out) {
    const FusedView V = slot_view(A, A.first + blockIdx.y);
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    int g = 0, ln = 0;
    float4 p;
    float r;
    unsigned long long h1 = 0, h2 = 0, h3 = 0, h4 = 0;
    if (fused_at(V, pos, g, p, r, ln)) {
        h1 = dg_mix(dg_key(g, 1) ^ (unsigned long long)V.label[pos]);
        h2 = dg_mix(dg_key(g, 2) ^ (unsigned long long)(ln & 255));
        h3 = dg_mix(dg_key(g, 3) ^ dg_pair(p.x, p.y)) + dg_mix(dg_key(g, 4) ^ dg_pair(p.z, p.w));
        h4 = dg_mix(dg_key(g, 5) ^ (unsigned long long)__float_as_uint(r));
    }
    unsigned long long* o = out + (size_t)blockIdx.y * MML_DIGEST_WORDS;
    dg_commit(h1, o + 1);
    dg_commit(h2, o + 2);
    dg_commit(h3, o + 3);
    dg_commit(h4, o + 4);
}
// pieces 0, 5-9: counts, stacks, factor records, pose (one stack entry per thread)
__global__ void __launch_bounds__(256) k_digest_stacks(DigestArgs A, unsigned long long* out) {
    const int slot = A.first + blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n0 = A.ft_n[slot], n1 = A.ft_n[A.B + slot];
    unsigned long long h5 = 0, h6 = 0, h7 = 0, h8 = 0;
    if (i < n0) {
        const float4 q = A.ft[0][(size_t)slot * A.MF + i];
        h5 = dg_mix(dg_key(i, 6) ^ dg_pair(q.x, q.y)) + dg_mix(dg_key(i, 8) ^ (unsigned long long)__float_as_uint(q.z));
        const MmlLineFactor f = A.lf[(size_t)slot * A.MF + i];
        if (f.src >= 0) {
            unsigned long long h = dg_key((unsigned)f.src, 10);
            for (int c = 0; c < 3; ++c) h = dg_mix(h ^ dg_dbits((double)f.ori[c]));
            for (int c = 0; c < 3; ++c) h = dg_mix(h ^ dg_dbits((double)f.p1[c]));
            for (int c = 0; c < 3; ++c) h = dg_mix(h ^ dg_dbits((double)f.p2[c]));
            h7 = dg_mix(h ^ dg_dbits(f.error));
        }
    }
    if (i < n1) {
        const float4 q = A.ft[1][(size_t)slot * A.MF + i];
        h6 = dg_mix(dg_key(i, 7) ^ dg_pair(q.x, q.y)) + dg_mix(dg_key(i, 9) ^ (unsigned long long)__float_as_uint(q.z));
        const MmlPlaneFactor f = A.pf[(size_t)slot * A.MF + i];
        if (f.src >= 0) {
            unsigned long long h = dg_key((unsigned)f.src, 11);
            for (int c = 0; c < 3; ++c) h = dg_mix(h ^ dg_dbits((double)f.ori[c]));
            for (int c = 0; c < 3; ++c) h = dg_mix(h ^ dg_dbits(f.proj[c]));
            for (int c = 0; c < 3; ++c) h = dg_mix(h ^ dg_dbits((double)f.omega[c]));
            h8 = dg_mix(h ^ dg_dbits(f.error));
        }
    }
    unsigned long long* o = out + (size_t)blockIdx.y * MML_DIGEST_WORDS;
    dg_commit(h5, o + 5);
    dg_commit(h6, o + 6);
    dg_commit(h7, o + 7);
    dg_commit(h8, o + 8);
    if (i == 0) {
        unsigned long long h = dg_key(0, 13);
        for (int c = 0; c < 6; ++c) h = dg_mix(h ^ (unsigned long long)(unsigned)A.fu_info[8 * (size_t)slot + c]);
        h = dg_mix(h ^ (unsigned long long)(unsigned)n0);
        h = dg_mix(h ^ (unsigned long long)(unsigned)n1);
        o[0] = h;
        unsigned long long hp = dg_key(0, 12);
        for (int c = 0; c < 6; ++c) hp = dg_mix(hp ^ dg_dbits(A.x[6 * (size_t)slot + c]));
        o[9] = hp;
    }
}
int ensure_wire_stage(mml_ctx* ctx, size_t bytes) { return ctx->wire_stage.reserve(ctx, bytes, MML_STREAM(ctx)); }
}  // namespace

namespace {
int upload_wire_impl(mml_ctx* ctx, int slot, const uint8_t* data, int n_points, int point_step, int off_x, int off_y,
                     int off_z, int off_intensity, const mml_livox_point* livox, const uint8_t* livox_wire, int n_livox);
}
int mml_scan_upload_pointcloud2(mml_ctx* ctx, int slot, const uint8_t* data, int n_points, int point_step, int off_x,
                                int off_y, int off_z, int off_intensity, const mml_livox_point* livox, int n_livox) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n_livox <= 0 || livox, MML_ERR_INVALID, "null point buffer");
    return upload_wire_impl(ctx, slot, data, n_points, point_step, off_x, off_y, off_z, off_intensity, livox, nullptr, n_livox);
}
int mml_scan_upload_wire(mml_ctx* ctx, int slot, const uint8_t* data, int n_points, int point_step, int off_x, int off_y,
                         int off_z, int off_intensity, const uint8_t* livox_wire, int n_livox) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n_livox <= 0 || livox_wire, MML_ERR_INVALID, "null point buffer");
    return upload_wire_impl(ctx, slot, data, n_points, point_step, off_x, off_y, off_z, off_intensity, nullptr, livox_wire, n_livox);
}
namespace {
int upload_wire_impl(mml_ctx* ctx, int slot, const uint8_t* data, int n_points, int point_step, int off_x, int off_y,
                     int off_z, int off_intensity, const mml_livox_point* livox, const uint8_t* livox_wire, int n_livox) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE(n_points >= 0 && n_livox >= 0, MML_ERR_INVALID, "negative point count");
    MML_REQUIRE(n_points <= ctx->cfg.max_velo_points && n_livox <= ctx->cfg.max_livox_points, MML_ERR_CAPACITY,
                "scan exceeds max_velo_points / max_livox_points");
    MML_REQUIRE(n_points == 0 || data, MML_ERR_INVALID, "null point buffer");
    MML_REQUIRE(point_step >= 12 && point_step <= 256, MML_ERR_INVALID, "point_step out of range");
    const int offs[4] = {off_x, off_y, off_z, off_intensity};
    for (int k = 0; k < 4; ++k)
        MML_REQUIRE((k == 3 && offs[k] < 0) || (offs[k] >= 0 && offs[k] + 4 <= point_step), MML_ERR_INVALID,
                    "field offset outside the point record");
    const size_t bytes = (size_t)n_points * point_step;
    const size_t lbytes = livox_wire ? (size_t)n_livox * 19 : 0;
    const size_t loff = (bytes + 15) & ~size_t(15);  // the Livox records follow the Velodyne payload in the staging buffer
    if (n_points || lbytes) {
        int rc = ensure_wire_stage(ctx, loff + lbytes);
        if (rc != MML_OK) return rc;
    }
    if (n_points) {
        MML_HIP(hipMemcpyAsync(ctx->wire_stage.d, data, bytes, hipMemcpyHostToDevice, MML_STREAM(ctx)));
        hipLaunchKernelGGL(k_decode_pointcloud2, dim3((n_points + 255) / 256), dim3(256), 0, MML_STREAM(ctx),
                           reinterpret_cast<const uint8_t*>(ctx->wire_stage.d), n_points, point_step, off_x, off_y, off_z,
                           off_intensity, ctx->velo_in + (size_t)slot * ctx->NV);
        MML_HIP(hipGetLastError());
    }
    // the Livox part: decoded from its wire form, or as in mml_scan_upload; the two counts travel as there
    if (n_livox && livox_wire) {
        uint8_t* dst = reinterpret_cast<uint8_t*>(ctx->wire_stage.d) + loff;
        MML_HIP(hipMemcpyAsync(dst, livox_wire, lbytes, hipMemcpyHostToDevice, MML_STREAM(ctx)));
        hipLaunchKernelGGL(k_decode_custompoints, dim3((n_livox + 255) / 256), dim3(256), 0, MML_STREAM(ctx), dst, n_livox,
                           ctx->livox_in + (size_t)slot * ctx->NL);
        MML_HIP(hipGetLastError());
    } else if (n_livox) {
        MML_HIP(hipMemcpyAsync(ctx->livox_in + (size_t)slot * ctx->NL, livox, sizeof(mml_livox_point) * (size_t)n_livox,
                               hipMemcpyHostToDevice, MML_STREAM(ctx)));
    }
    ctx->h_n_in[2 * slot] = n_points;
    ctx->raw_extracted[slot] = 0;
    ctx->h_n_in[2 * slot + 1] = n_livox;
    double* st = stage_alloc(ctx, 1);
    int* sti = reinterpret_cast<int*>(st);
    sti[0] = n_points;
    sti[1] = n_livox;
    MML_HIP(hipMemcpyAsync(ctx->d_n_in + 2 * slot, sti, sizeof(int) * 2, hipMemcpyHostToDevice, MML_STREAM(ctx)));
    return MML_OK;
}
}  // namespace

namespace {
int fused_view(mml_ctx* ctx, int slot, FusedView& V) {
    int fl = 0;
    MML_HIP(hipMemcpyAsync(&fl, ctx->slot_flags + 2 * (size_t)slot, sizeof(int), hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    const size_t off = (size_t)slot * ctx->NT;
    V.pts = ctx->ln_pts + off;
    V.gidx = ctx->ln_gidx + off;
    V.rel = ctx->ln_rel + off;
    V.line = ctx->ln_line + off;
    V.label = ctx->ln_label + off;
    V.cb_n = ctx->cb_n + 2 * (size_t)slot;
    V.seg_flat = ctx->seg_flat + (size_t)slot * 2 * MML_SEG_FLAT;
    V.seg_flat_n = ctx->seg_flat_n + (size_t)slot * 4;
    V.NV = ctx->NV;
    V.NT = ctx->NT;
    V.L = ctx->L;
    V.n_rings = ctx->cfg.n_rings;
    V.flags = fl;
    return MML_OK;
}
}  // namespace

int mml_scan_download_pointxyzinormal(mml_ctx* ctx, int slot, uint8_t* out, int capacity_points, int* n_points) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE(n_points != nullptr, MML_ERR_INVALID, "null n_points");
    int rc = mml_cloud_settle(ctx, slot, 1);
    if (rc != MML_OK) return rc;
    mml_scan_info info;
    rc = mml_scan_info_get(ctx, slot, &info);
    if (rc != MML_OK) return rc;
    *n_points = info.n_points;
    if (!out || info.n_points == 0) return MML_OK;
    MML_REQUIRE(capacity_points >= info.n_points, MML_ERR_CAPACITY, "download capacity too small");
    const size_t bytes = (size_t)info.n_points * 48;
    rc = ensure_wire_stage(ctx, bytes);
    if (rc != MML_OK) return rc;
    FusedView V;
    rc = fused_view(ctx, slot, V);
    if (rc != MML_OK) return rc;
    hipLaunchKernelGGL(k_encode_xyzinormal, dim3((ctx->NT + 255) / 256), dim3(256), 0, MML_STREAM(ctx), V,
                       reinterpret_cast<float*>(ctx->wire_stage.d));
    MML_HIP(hipGetLastError());
    MML_HIP(hipMemcpyAsync(out, ctx->wire_stage.d, bytes, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    return MML_OK;
}

int mml_cloud_download_registered_batch(mml_ctx* ctx, int first_slot, int count, const double* T_wl, uint8_t* out,
                                        long capacity_points, int* n_points) {
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(T_wl != nullptr && n_points != nullptr, MML_ERR_INVALID, "null T_wl / n_points");
    MML_REQUIRE(count <= 65535, MML_ERR_INVALID, "at most 65535 slots per call (the grid's second dimension)");
    int rc = mml_cloud_settle(ctx, first_slot, count);
    if (rc != MML_OK) return rc;
    // synchronisation 1 of 2: the counts of all slots in one copy (the flag words stay on the device, slot_view reads them)
    double* st = stage_alloc(ctx, 21 * (size_t)count);  // pinned: 8 ints per slot back, then 16 + 1 doubles per slot down
    int* h_info = reinterpret_cast<int*>(st);
    MML_HIP(hipMemcpyAsync(h_info, ctx->fu_info + 8 * (size_t)first_slot, sizeof(int) * 8 * (size_t)count, hipMemcpyDeviceToHost,
                           MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    long long total = 0;
    for (int i = 0; i < count; ++i) total += (n_points[i] = h_info[8 * i]);
    if (!out) return MML_OK;
    MML_REQUIRE(capacity_points >= total, MML_ERR_CAPACITY, "download capacity too small");
    if (total == 0) return MML_OK;
    const size_t bytes = (size_t)total * 48;
    rc = ensure_wire_stage(ctx, bytes);
    if (rc != MML_OK) return rc;
    // poses, then record offsets (the exclusive prefix sum of the counts), down in one copy into the call's slice of d_pose_in
    double* h_par = st + 4 * (size_t)count;
    memcpy(h_par, T_wl, sizeof(double) * 16 * (size_t)count);
    long long* h_off = reinterpret_cast<long long*>(h_par + 16 * (size_t)count);
    long long run = 0;
    for (int i = 0; i < count; ++i) {
        h_off[i] = run;
        run += h_info[8 * i];
    }
    double* d_par = ctx->d_pose_in + kPoseSlotDoubles * (size_t)first_slot;
    MML_HIP(hipMemcpyAsync(d_par, h_par, sizeof(double) * 17 * (size_t)count, hipMemcpyHostToDevice, MML_STREAM(ctx)));
    const SlotArrays A = slot_arrays(ctx, first_slot);
    hipLaunchKernelGGL(k_encode_registered, dim3((ctx->NT + 255) / 256, count), dim3(256), 0, MML_STREAM(ctx), A, d_par, count,
                       reinterpret_cast<float4*>(ctx->wire_stage.d));
    MML_HIP(hipGetLastError());
    // synchronisation 2 of 2: the records
    MML_HIP(hipMemcpyAsync(out, ctx->wire_stage.d, bytes, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    return MML_OK;
}

int mml_cloud_download_registered(mml_ctx* ctx, int slot, const double* T_wl, uint8_t* out, int capacity_points, int* n_points) {
    return mml_cloud_download_registered_batch(ctx, slot, 1, T_wl, out, capacity_points, n_points);
}

// Table block of mml_feature_clouds_download_batch (device + pinned twin), grow-only, owned by the context: the call drains the
// stream before it returns, so reserve() never replaces a buffer in use.
struct MmlFeatCloudsDev {
    MmlStaging<char> io;
    ~MmlFeatCloudsDev() { io.release(); }
};
namespace {
struct FeatCloudsIo {
    MmlCarve<16> c;
    MmlField<int> fi, fl;      // up: the slots' counters and state flags
    MmlField<long long> off;   // down: where every cloud starts, and the total
    MmlField<int> got;         // up: what the raw-order walk found
    size_t bytes;
    explicit FeatCloudsIo(size_t n) : fi(c.take<int>(8 * n)), fl(c.take<int>(2 * n)), off(c.take<long long>(6 * n + 1)), got(c.take<int>(6 * n)), bytes(c.bytes()) {}
};
}  // namespace

int mml_feature_clouds_download_batch(mml_ctx* ctx, int first_slot, int count, uint8_t* out, long capacity_points, int* n_points) {
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(n_points != nullptr, MML_ERR_INVALID, "null n_points");
    MML_REQUIRE(count <= 65535, MML_ERR_INVALID, "at most 65535 slots per call (the grid's second dimension)");
    const char* who = "mml_feature_clouds_download_batch";
    // the raw-order clouds are those of the EXTRACTED scan: raw_line is re-derived from the raw records (mml_gicp_refresh's rule)
    for (int i = 0; i < count; ++i)
        if (!ctx->raw_extracted[first_slot + i])
            return mml_refuse(ctx, MML_ERR_STATE, "%s: slot %d's raw scan was re-uploaded after mml_extract (or never extracted)", who, first_slot + i);
    hipStream_t s = MML_STREAM(ctx);
    const size_t n = (size_t)count, f = (size_t)first_slot;
    const FeatCloudsIo io(n);
    MmlFeatCloudsDev* d = mml_side<MmlFeatCloudsDev>(ctx, MML_SIDE_FEATURE_CLOUDS);
    if (d->io.reserve(ctx, io.bytes, s)) return MML_ERR_HIP;
    char *h = d->io.h, *g = d->io.d;
    // synchronisation 1 of 2: counters and state flags of all slots
    const int *fi = io.fi.in(h), *fl = io.fl.in(h);
    MML_HIP(hipMemcpyAsync(io.fi.in(h), ctx->fu_info + 8 * f, io.fi.bytes(), hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(io.fl.in(h), ctx->slot_flags + 2 * f, io.fl.bytes(), hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < count; ++i)
        if ((fl[2 * i] & 3) != 0)
            return mml_refuse(ctx, MML_ERR_STATE, "%s: slot %d holds an uploaded or undistorted cloud (call it after mml_extract, before mml_undistort)",
                              who, first_slot + i);
    long long* off = io.off.in(h);
    long long total = 0;
    for (int i = 0; i < count; ++i) {
        const int* c = fi + 8 * i;  // n_points, n_velo, velo_corner_num, velo_surf_num, livox_corner_num, livox_surf_num
        const int np[6] = {c[2], c[3], c[1], c[4], c[5], c[0] - c[1]};
        for (int k = 0; k < 6; ++k) {
            off[6 * i + k] = total;
            total += (n_points[6 * i + k] = np[k]);
        }
    }
    off[6 * n] = total;
    if (!out) return MML_OK;
    MML_REQUIRE(capacity_points >= total, MML_ERR_CAPACITY, "download capacity too small");
    if (total == 0) return MML_OK;
    const size_t bytes = (size_t)total * 48;
    int rc = ensure_wire_stage(ctx, bytes);
    if (rc != MML_OK) return rc;
    float4* rec = reinterpret_cast<float4*>(ctx->wire_stage.d);
    MML_HIP(hipMemcpyAsync(io.off.in(g), off, io.off.bytes(), hipMemcpyHostToDevice, s));
    // (the one-pass bucketing keeps no per-point line ids: recomputed from the raw buffers, which raw_extracted pins -- raw_line,
    //  raw_ori and blk_cnt are rewritten with the values they already hold)
    if (ctx->onepass) {
        rc = mml_launch_raw_lines(ctx, first_slot, count);
        if (rc != MML_OK) return rc;
    }
    const FeatCloudArgs A{ctx->raw_line, ctx->d_n_in, ctx->seg_flat, ctx->seg_flat_n, ctx->ln_label, ctx->ln_rel, ctx->velo_in, ctx->livox_in,
                          first_slot,    ctx->NT,     ctx->NV,       ctx->NL,         ctx->onepass ? MML_OP_BLK : (1 << 30)};
    hipLaunchKernelGGL(k_feature_gather, dim3(2, count), dim3(RG_THREADS), 0, s, A, io.off.in(g), rec, io.got.in(g));
    hipLaunchKernelGGL(k_encode_combine, dim3((ctx->NT + 255) / 256, count), dim3(256), 0, s, slot_arrays(ctx, first_slot), io.off.in(g), rec);
    MML_HIP(hipGetLastError());
    // synchronisation 2 of 2: the records, and the walk's own counts
    MML_HIP(hipMemcpyAsync(io.got.in(h), io.got.in(g), io.got.bytes(), hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(out, ctx->wire_stage.d, bytes, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    const int* got = io.got.in(h);
    for (int i = 0; i < count; ++i)
        for (int k = 0; k < 6; ++k)
            if (k % 3 != 2 && got[6 * i + k] != n_points[6 * i + k])
                return mml_refuse(ctx, MML_ERR_STATE, "%s: slot %d, cloud %d: %d labelled points in raw order against a counter of %d", who, first_slot + i, k,
                                  got[6 * i + k], n_points[6 * i + k]);
    return MML_OK;
}

int mml_feature_clouds_download(mml_ctx* ctx, int slot, uint8_t* out, int capacity_points, int* n_points) {
    return mml_feature_clouds_download_batch(ctx, slot, 1, out, capacity_points, n_points);
}

int mml_cloud_upload(mml_ctx* ctx, int slot, const uint8_t* pointxyzinormal, int n_points, int n_velo) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE(n_points >= 0 && n_velo >= 0 && n_velo <= n_points, MML_ERR_INVALID, "bad point counts");
    MML_REQUIRE(n_points == 0 || pointxyzinormal, MML_ERR_INVALID, "null point buffer");
    MML_REQUIRE(n_velo <= ctx->NV && n_points - n_velo <= ctx->NL, MML_ERR_CAPACITY,
                "cloud exceeds max_velo_points / max_livox_points (the Velodyne and Livox parts have their own regions)");
    const size_t bytes = (size_t)n_points * 48;
    int rc = ensure_wire_stage(ctx, bytes ? bytes : 48);
    if (rc != MML_OK) return rc;
    if (bytes) MML_HIP(hipMemcpyAsync(ctx->wire_stage.d, pointxyzinormal, bytes, hipMemcpyHostToDevice, MML_STREAM(ctx)));
    ctx->und_pending[slot] = 0;  // (the cloud is replaced: nothing of the old one is left to finish)
    rc = mml_launch_cloud_decode(ctx, slot, reinterpret_cast<const float*>(ctx->wire_stage.d), n_points, n_velo);
    if (rc != MML_OK) return rc;
    // the staging buffer is reused by the next wire-format call and the host buffer belongs to the caller
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    return MML_OK;
}

int mml_extract(mml_ctx* ctx, int first_slot, int count, const float* livox_extrinsic) {
    CHECK_SLOTS(first_slot, count);
    bool have = false;
    if (livox_extrinsic) {
        static const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        have = memcmp(I, livox_extrinsic, sizeof(I)) != 0;
        if (have) {
            double* st = stage_alloc(ctx, 8);
            memcpy(st, livox_extrinsic, sizeof(float) * 16);
            MML_HIP(hipMemcpyAsync(ctx->d_extr, st, sizeof(float) * 16, hipMemcpyHostToDevice, MML_STREAM(ctx)));
        }
    }
    return mml_launch_extract(ctx, first_slot, count, have);
}

int mml_scan_info_get(mml_ctx* ctx, int slot, mml_scan_info* info) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE(info != nullptr, MML_ERR_INVALID, "null info");
    int* h = reinterpret_cast<int*>(stage_alloc(ctx, 4));  // pinned: a pageable destination makes the copy a blocking staged one
    MML_HIP(hipMemcpyAsync(h, ctx->fu_info + 8 * slot, sizeof(int) * 8, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    info->n_points = h[0];
    info->n_velo = h[1];
    info->velo_corner_num = h[2];
    info->velo_surf_num = h[3];
    info->livox_corner_num = h[4];
    info->livox_surf_num = h[5];
    info->fused_corner_num = h[6];
    info->fused_surf_num = h[7];
    return MML_OK;
}

int mml_scan_download(mml_ctx* ctx, int slot, float* xyzi, float* reltime, uint8_t* line, uint8_t* label,
                      int capacity) {
    CHECK_SLOTS(slot, 1);
    int rc = mml_cloud_settle(ctx, slot, 1);
    if (rc != MML_OK) return rc;
    mml_scan_info info;
    rc = mml_scan_info_get(ctx, slot, &info);
    if (rc != MML_OK) return rc;
    MML_REQUIRE(capacity >= info.n_points, MML_ERR_CAPACITY, "download capacity too small");
    const size_t n = info.n_points;
    if (n == 0) return MML_OK;
    // the fused order exists only here: gathered into a staging buffer (16 + 4 + 1 + 1 bytes per point), then copied out
    const size_t n16 = (n + 15) & ~size_t(15);
    rc = ensure_wire_stage(ctx, n16 * 22);
    if (rc != MML_OK) return rc;
    uint8_t* st = reinterpret_cast<uint8_t*>(ctx->wire_stage.d);
    float4* s_xyzi = reinterpret_cast<float4*>(st);
    float* s_rel = reinterpret_cast<float*>(st + n16 * 16);
    uint8_t* s_line = st + n16 * 20;
    uint8_t* s_label = st + n16 * 21;
    FusedView V;
    rc = fused_view(ctx, slot, V);
    if (rc != MML_OK) return rc;
    hipLaunchKernelGGL(k_fused_arrays, dim3((ctx->NT + 255) / 256), dim3(256), 0, MML_STREAM(ctx), V, (int)n, s_xyzi, s_rel, s_line, s_label);
    MML_HIP(hipGetLastError());
    if (xyzi) MML_HIP(hipMemcpyAsync(xyzi, s_xyzi, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    if (reltime) MML_HIP(hipMemcpyAsync(reltime, s_rel, sizeof(float) * n, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    if (line) MML_HIP(hipMemcpyAsync(line, s_line, n, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    if (label) MML_HIP(hipMemcpyAsync(label, s_label, n, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    return MML_OK;
}

int mml_slot_digest(mml_ctx* ctx, int first_slot, int count, uint64_t* out) {
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(out != nullptr, MML_ERR_INVALID, "null out");
    int rc = mml_sync_all(ctx);
    if (rc != MML_OK) return rc;
    rc = mml_cloud_settle(ctx, first_slot, count);
    if (rc != MML_OK) return rc;
    MmlTemp<unsigned long long> tmp;
    const size_t bytes = sizeof(unsigned long long) * MML_DIGEST_WORDS * (size_t)count;
    MML_HIP(tmp.alloc(MML_DIGEST_WORDS * (size_t)count));
    unsigned long long* d = tmp.d;
    hipError_t e = hipMemsetAsync(d, 0, bytes, MML_STREAM(ctx));
    DigestArgs A;
    static_cast<SlotArrays&>(A) = slot_arrays(ctx, first_slot);
    A.ft_n = ctx->ft_n;
    A.ft[0] = ctx->ft_xyz[0];
    A.ft[1] = ctx->ft_xyz[1];
    A.lf = ctx->lf;
    A.pf = ctx->pf;
    A.x = ctx->d_x;
    A.B = ctx->B;
    A.MF = ctx->MF;
    // (gridDim.y is limited to 65535: calls of more slots go in pieces)
    for (int done = 0; done < count && e == hipSuccess; done += 32768) {
        const int c = std::min(32768, count - done);
        A.first = first_slot + done;
        unsigned long long* o = d + (size_t)done * MML_DIGEST_WORDS;
        hipLaunchKernelGGL(k_digest_cloud, dim3((ctx->NT + 255) / 256, c), dim3(256), 0, MML_STREAM(ctx), A, o);
        hipLaunchKernelGGL(k_digest_stacks, dim3((ctx->MF + 255) / 256, c), dim3(256), 0, MML_STREAM(ctx), A, o);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, MML_STREAM(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(MML_STREAM(ctx));
    if (e != hipSuccess) {
        ctx->err = std::string("mml_slot_digest: ") + hipGetErrorString(e);
        return MML_ERR_HIP;
    }
    return MML_OK;
}

int mml_detect_line(mml_ctx* ctx, const float* pts, int n, int* sharp, int* n_sharp, int* flat, int* n_flat,
                    int* flags) {
    CHECK_SLOTS(0, 1);
    MML_REQUIRE(n >= 0 && n_sharp && n_flat && (n == 0 || (pts && sharp && flat)), MML_ERR_INVALID, "bad arguments");
    MML_REQUIRE(n <= ctx->NV, MML_ERR_CAPACITY, "line longer than max_velo_points");
    *n_sharp = 0;
    *n_flat = 0;
    if (n == 0) return MML_OK;
    {  // (slot 0 is this call's scratch: what it leaves of the slot's cloud is what it left before there were partly undistorted slots)
        int rc0 = mml_cloud_settle(ctx, 0, 1);
        if (rc0 != MML_OK) return rc0;
    }
    for (int i = 0; i < n; ++i)
        MML_REQUIRE(std::isfinite(pts[4 * i]) && std::isfinite(pts[4 * i + 1]) && std::isfinite(pts[4 * i + 2]),
                    MML_ERR_INVALID, "detectFeaturePoints: non-finite input (reference indexes pre-compaction)");
    MML_HIP(hipMemcpyAsync(ctx->ln_pts, pts, sizeof(float) * 4 * (size_t)n, hipMemcpyHostToDevice, MML_STREAM(ctx)));
    // ln_final scratch: reuse ln_ord_c of slot 0's livox region?  Use a dedicated view of raw_ori (NV floats >= n*2 bytes).
    uint16_t* d_final = reinterpret_cast<uint16_t*>(ctx->raw_ori);
    int rc = mml_launch_detect_line(ctx, n, d_final);
    if (rc != MML_OK) return rc;
    std::vector<uint8_t> lab(n);
    std::vector<uint16_t> fin(n);
    MML_HIP(hipMemcpyAsync(lab.data(), ctx->ln_label, n, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipMemcpyAsync(fin.data(), d_final, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    int ns = 0, nf = 0;
    for (int i = 0; i < n; ++i) {  // ascending i, as the emit loop at unionFeatureExtract.cpp:818-842
        if (lab[i] == 2) flat[nf++] = i;
        if (lab[i] == 1) sharp[ns++] = i;
        if (flags) flags[i] = fin[i];
    }
    *n_sharp = ns;
    *n_flat = nf;
    return MML_OK;
}

int mml_undistort(mml_ctx* ctx, int first_slot, int count, const double* dR, const double* dt) {
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(dR && dt, MML_ERR_INVALID, "null dR/dt");
    int rc = mml_cloud_settle(ctx, first_slot, count);  // (a second undistortion starts from a complete first one)
    if (rc != MML_OK) return rc;
    double* st = stage_alloc(ctx, 12 * (size_t)count);  // the sweep motions, at the start of the slots' range of d_pose_in
    for (int i = 0; i < count; ++i) {
        memcpy(st + 12 * i, dR + 9 * i, sizeof(double) * 9);
        memcpy(st + 12 * i + 9, dt + 3 * i, sizeof(double) * 3);
    }
    double* d_par = ctx->d_pose_in + kPoseSlotDoubles * (size_t)first_slot;
    MML_HIP(hipMemcpyAsync(d_par, st, sizeof(double) * 12 * count, hipMemcpyHostToDevice, MML_STREAM(ctx)));
    return mml_launch_undistort(ctx, first_slot, count, d_par);
}

int mml_downsample(mml_ctx* ctx, int first_slot, int count) {
    CHECK_SLOTS(first_slot, count);
    int rc = mml_cloud_settle(ctx, first_slot, count);
    if (rc != MML_OK) return rc;
    rc = mml_launch_downsample(ctx, first_slot, count);
    if (rc != MML_OK) return rc;
    // pcl::VoxelGrid takes a cloud of any size: slots whose labelled cloud is beyond the LDS sort are redone
    return mml_downsample_redo_overflow(ctx, first_slot, count, nullptr);
}

int mml_features_download(mml_ctx* ctx, int slot, int kind, float* xyz, int capacity, int* n) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE((kind == 0 || kind == 1) && n, MML_ERR_INVALID, "bad kind");
    int h = 0;
    MML_HIP(hipMemcpyAsync(&h, ctx->ft_n + kind * ctx->B + slot, sizeof(int), hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    MML_REQUIRE(h >= 0, MML_ERR_CAPACITY, "down-sample overflowed max_features / voxel capacity");
    *n = h;
    if (!xyz || h == 0) return MML_OK;
    MML_REQUIRE(capacity >= h, MML_ERR_CAPACITY, "download capacity too small");
    std::vector<float4> tmp(h);
    MML_HIP(hipMemcpyAsync(tmp.data(), ctx->ft_xyz[kind] + (size_t)slot * ctx->MF, sizeof(float4) * h,
                           hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    for (int i = 0; i < h; ++i) {
        xyz[3 * i] = tmp[i].x;
        xyz[3 * i + 1] = tmp[i].y;
        xyz[3 * i + 2] = tmp[i].z;
    }
    return MML_OK;
}

int mml_features_upload(mml_ctx* ctx, int slot, int kind, const float* xyz, int n) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE((kind == 0 || kind == 1) && n >= 0 && (n == 0 || xyz), MML_ERR_INVALID, "bad arguments");
    MML_REQUIRE(n <= ctx->MF, MML_ERR_CAPACITY, "more features than max_features");
    std::vector<float4> tmp(n ? n : 1);
    for (int i = 0; i < n; ++i) tmp[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.f);
    if (n)
        MML_HIP(hipMemcpyAsync(ctx->ft_xyz[kind] + (size_t)slot * ctx->MF, tmp.data(), sizeof(float4) * n,
                               hipMemcpyHostToDevice, MML_STREAM(ctx)));
    MML_HIP(hipMemcpyAsync(ctx->ft_n + kind * ctx->B + slot, &n, sizeof(int), hipMemcpyHostToDevice, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    return MML_OK;
}

// (the map calls -- mml_map_set_local ... mml_map_set_global -- live in map_banks.hip, beside the banks' forms of them)

int mml_knn5(mml_ctx* ctx, int kind, const float* q, int nq, float max_d2, int* idx, float* d2) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE((kind == 0 || kind == 1) && nq >= 0 && (nq == 0 || (q && idx && d2)), MML_ERR_INVALID, "bad arguments");
    MML_REQUIRE(ctx->own.have_map[kind], MML_ERR_STATE, "mml_knn5 before mml_map_set_local");
    if (nq == 0) return MML_OK;
    MML_HIP(hipSetDevice(ctx->device));
    MmlTemp<float> d_q, d_d2;
    MmlTemp<int> d_idx;
    MML_HIP(d_q.alloc(3 * (size_t)nq));
    MML_HIP(d_idx.alloc(5 * (size_t)nq));
    MML_HIP(d_d2.alloc(5 * (size_t)nq));
    MML_HIP(hipMemcpyAsync(d_q.d, q, sizeof(float) * 3 * nq, hipMemcpyHostToDevice, MML_STREAM(ctx)));
    int rc = mml_launch_knn5(ctx, kind, d_q.d, nq, max_d2, d_idx.d, d_d2.d);
    if (rc == MML_OK) {
        hipMemcpyAsync(idx, d_idx.d, sizeof(int) * 5 * nq, hipMemcpyDeviceToHost, MML_STREAM(ctx));
        hipMemcpyAsync(d2, d_d2.d, sizeof(float) * 5 * nq, hipMemcpyDeviceToHost, MML_STREAM(ctx));
    }
    hipError_t e = hipStreamSynchronize(MML_STREAM(ctx));
    if (e != hipSuccess) {
        ctx->err = std::string("mml_knn5: ") + hipGetErrorString(e);
        return MML_ERR_HIP;
    }
    return rc;
}

static void finish_stats(const double* s, mml_assoc_stats* o) {
    o->n_line = (int)s[0];
    o->n_plane = (int)s[1];
    o->n_line_used = (int)s[2];
    o->n_plane_used = (int)s[3];
    for (int k = 0; k < 9; ++k) o->normal_gram[k] = s[4 + k];
    // checkLocalizability (Estimator.cpp:536-565): smallest singular value of the M x 3 normal matrix =
    // sqrt(lambda_min(gram)); 3x3 symmetric eigenvalues by the trigonometric closed form (host, once per call)
    if (!(o->n_plane > 10)) {
        o->min_singular = -1;
    } else {
        const double* A = o->normal_gram;
        double p1 = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
        double lam_min;
        double q = (A[0] + A[4] + A[8]) / 3.0;
        double p2 = (A[0] - q) * (A[0] - q) + (A[4] - q) * (A[4] - q) + (A[8] - q) * (A[8] - q) + 2 * p1;
        double p = sqrt(p2 / 6.0);
        if (p < 1e-300) {
            lam_min = q;
        } else {
            double Bm[9];
            for (int k = 0; k < 9; ++k) Bm[k] = (A[k] - ((k % 4 == 0) ? q : 0.0)) / p;
            double detB = Bm[0] * (Bm[4] * Bm[8] - Bm[5] * Bm[7]) - Bm[1] * (Bm[3] * Bm[8] - Bm[5] * Bm[6]) +
                          Bm[2] * (Bm[3] * Bm[7] - Bm[4] * Bm[6]);
            double r = detB / 2.0;
            r = r < -1 ? -1 : (r > 1 ? 1 : r);
            double phi = acos(r) / 3.0;
            lam_min = q + 2 * p * cos(phi + 2.0 * M_PI / 3.0);
        }
        o->min_singular = sqrt(lam_min > 0 ? lam_min : 0.0);
    }
    o->is_degenerate = o->min_singular < 3.0 ? 1 : 0;  // Estimator.cpp:772-775
}

int mml_associate(mml_ctx* ctx, int first_slot, int count, const double* T_wl, double thres_dist,
                  mml_assoc_stats* stats) {
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(T_wl != nullptr, MML_ERR_INVALID, "null T_wl");
    {
        const int ready = mml_assoc_ready(ctx, first_slot, count, "mml_associate");
        if (ready != MML_OK) return ready;
    }
    double* d_T = ctx->d_pose_in + kPoseSlotDoubles * (size_t)first_slot;
    int rc = upload_doubles(ctx, d_T, T_wl, 16 * (size_t)count);
    if (rc != MML_OK) return rc;
    rc = mml_launch_associate(ctx, first_slot, count, d_T, thres_dist, true);
    if (rc != MML_OK) return rc;
    if (stats) {
        double* h = stage_alloc(ctx, 16 * (size_t)count);  // pinned
        MML_HIP(hipMemcpyAsync(h, ctx->assoc_stats + 16 * (size_t)first_slot, sizeof(double) * 16 * (size_t)count,
                               hipMemcpyDeviceToHost, MML_STREAM(ctx)));
        MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
        for (int i = 0; i < count; ++i) finish_stats(h + 16 * i, &stats[i]);
    }
    return MML_OK;
}

int mml_factors_upload(mml_ctx* ctx, int slot, int kind, const double* rec, int n) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE((kind == 0 || kind == 1) && n >= 0 && (n == 0 || rec), MML_ERR_INVALID, "bad arguments");
    MML_REQUIRE(n <= ctx->MF, MML_ERR_CAPACITY, "more factors than max_features");
    ctx->stats_stale[slot] = 1;  // (the slot's statistics no longer describe its factors: recomputed when asked for)
    if (kind == 0) {
        std::vector<MmlLineFactor> h(n ? n : 1);
        for (int i = 0; i < n; ++i) {
            const double* r = rec + 10 * (size_t)i;
            for (int c = 0; c < 3; ++c) {
                h[i].ori[c] = (float)r[c];
                h[i].p1[c] = (float)r[3 + c];
                h[i].p2[c] = (float)r[6 + c];
            }
            h[i].src = i;
            h[i].error = r[9];
        }
        if (n) MML_HIP(hipMemcpyAsync(ctx->lf + (size_t)slot * ctx->MF, h.data(), sizeof(MmlLineFactor) * n, hipMemcpyHostToDevice, MML_STREAM(ctx)));
        MML_HIP(hipMemcpyAsync(ctx->ft_n + slot, &n, sizeof(int), hipMemcpyHostToDevice, MML_STREAM(ctx)));
        MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));  // (the staging vector goes out of scope)
    } else {
        std::vector<MmlPlaneFactor> h(n ? n : 1);
        for (int i = 0; i < n; ++i) {
            const double* r = rec + 10 * (size_t)i;
            for (int c = 0; c < 3; ++c) {
                h[i].ori[c] = (float)r[c];
                h[i].proj[c] = r[3 + c];
                h[i].omega[c] = (float)r[6 + c];
            }
            h[i].src = i;
            h[i]._pad = 0;
            h[i].error = r[9];
        }
        if (n) MML_HIP(hipMemcpyAsync(ctx->pf + (size_t)slot * ctx->MF, h.data(), sizeof(MmlPlaneFactor) * n, hipMemcpyHostToDevice, MML_STREAM(ctx)));
        MML_HIP(hipMemcpyAsync(ctx->ft_n + ctx->B + slot, &n, sizeof(int), hipMemcpyHostToDevice, MML_STREAM(ctx)));
        MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    }
    return MML_OK;
}

int mml_factors_download(mml_ctx* ctx, int slot, int kind, double* out, int* src, int capacity, int* n) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE((kind == 0 || kind == 1) && n, MML_ERR_INVALID, "bad arguments");
    int nf = 0;
    MML_HIP(hipMemcpyAsync(&nf, ctx->ft_n + kind * ctx->B + slot, sizeof(int), hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    MML_REQUIRE(nf >= 0, MML_ERR_CAPACITY, "feature stack overflowed");
    int cnt = 0;
    if (kind == 0) {
        std::vector<MmlLineFactor> h(nf ? nf : 1);
        if (nf) MML_HIP(hipMemcpy(h.data(), ctx->lf + (size_t)slot * ctx->MF, sizeof(MmlLineFactor) * nf, hipMemcpyDeviceToHost));
        for (int i = 0; i < nf; ++i) {
            if (h[i].src < 0) continue;
            if (cnt < capacity && out) {
                double* o = out + 10 * cnt;
                for (int c = 0; c < 3; ++c) {
                    o[c] = h[i].ori[c];
                    o[3 + c] = h[i].p1[c];
                    o[6 + c] = h[i].p2[c];
                }
                o[9] = h[i].error;
                if (src) src[cnt] = h[i].src;
            }
            ++cnt;
        }
    } else {
        std::vector<MmlPlaneFactor> h(nf ? nf : 1);
        if (nf) MML_HIP(hipMemcpy(h.data(), ctx->pf + (size_t)slot * ctx->MF, sizeof(MmlPlaneFactor) * nf, hipMemcpyDeviceToHost));
        for (int i = 0; i < nf; ++i) {
            if (h[i].src < 0) continue;
            if (cnt < capacity && out) {
                double* o = out + 10 * cnt;
                for (int c = 0; c < 3; ++c) {
                    o[c] = h[i].ori[c];
                    o[3 + c] = h[i].proj[c];
                    o[6 + c] = h[i].omega[c];
                }
                o[9] = h[i].error;
                if (src) src[cnt] = h[i].src;
            }
            ++cnt;
        }
    }
    *n = cnt;
    MML_REQUIRE(!out || cnt <= capacity, MML_ERR_CAPACITY, "factor download capacity too small");
    return MML_OK;
}

int mml_linearize_record(mml_ctx* ctx, int slot, const double* x, const double* T_bl, double plan_weight_tan,
                         double huber_delta, double* d_record) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE(x && T_bl && d_record, MML_ERR_INVALID, "null argument");
    double h[22];
    memcpy(h, x, sizeof(double) * 6);
    memcpy(h + 6, T_bl, sizeof(double) * 16);
    double* d_par = ctx->d_pose_in + kPoseSlotDoubles * (size_t)slot;
    int rc = upload_doubles(ctx, d_par, h, 22);
    if (rc != MML_OK) return rc;
    return mml_launch_linearize(ctx, slot, d_par, d_par + 6, plan_weight_tan, huber_delta, d_record);
}

int mml_linearize_window(mml_ctx* ctx, int first_slot, int frames, int x_stride, const double* x, const double* T_bl,
                         double plan_weight_tan, double huber_delta, double* records) {
    CHECK_SLOTS(first_slot, frames);
    MML_REQUIRE(x && T_bl && records && x_stride >= 6 && frames <= 8, MML_ERR_INVALID, "bad arguments");
    double h[6 * 8 + 16];
    for (int f = 0; f < frames; ++f) memcpy(h + 6 * f, x + (size_t)x_stride * f, sizeof(double) * 6);
    memcpy(h + 6 * frames, T_bl, sizeof(double) * 16);
    // 64 doubles of parameter space per slot: poses of the window, then T_bl, in the first slot's block
    double* d_par = ctx->d_pose_in + kPoseSlotDoubles * (size_t)first_slot;
    int rc = upload_doubles(ctx, d_par, h, 6 * (size_t)frames + 16);
    if (rc != MML_OK) return rc;
    double* d_rec = ctx->d_rec + 32 * (size_t)first_slot;
    rc = mml_launch_linearize(ctx, first_slot, d_par, d_par + 6 * frames, plan_weight_tan, huber_delta, d_rec, frames);
    if (rc != MML_OK) return rc;
    MML_HIP(hipMemcpyAsync(records, d_rec, sizeof(double) * 32 * frames, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    return MML_OK;
}

int mml_linearize(mml_ctx* ctx, int slot, const double* x, const double* T_bl, double plan_weight_tan,
                  double huber_delta, double* H, double* g, double* cost) {
    CHECK_SLOTS(slot, 1);
    MML_REQUIRE(H && g && cost, MML_ERR_INVALID, "null output");
    double* d_rec = ctx->d_rec + 32 * (size_t)slot;
    int rc = mml_linearize_record(ctx, slot, x, T_bl, plan_weight_tan, huber_delta, d_rec);
    if (rc != MML_OK) return rc;
    double rec[32];
    MML_HIP(hipMemcpyAsync(rec, d_rec, sizeof(rec), hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) {
            H[6 * a + b] = rec[k];
            H[6 * b + a] = rec[k];
            ++k;
        }
    for (int a = 0; a < 6; ++a) g[a] = rec[21 + a];
    *cost = rec[27];
    return MML_OK;
}

int mml_solve(mml_ctx* ctx, int first_slot, int count, int window, const double* T_bl, const mml_solve_opts* opts,
              double* x, mml_solve_summary* summaries, double* trace) {
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(T_bl && opts && x, MML_ERR_INVALID, "null argument");
    MML_REQUIRE(opts->max_num_iterations >= 0 && opts->max_num_iterations <= 64, MML_ERR_INVALID,
                "max_num_iterations must be in [0, 64]");
    int rc = upload_doubles(ctx, ctx->d_x + 6 * (size_t)first_slot, x, 6 * (size_t)count);
    if (rc != MML_OK) return rc;
    double* d_Tbl = ctx->d_pose_in + kPoseSlotDoubles * (size_t)(first_slot + count) - 16;  // tail of this call's range
    rc = upload_doubles(ctx, d_Tbl, T_bl, 16);
    if (rc != MML_OK) return rc;
    rc = mml_launch_solve(ctx, first_slot, count, window, d_Tbl, *opts, trace != nullptr);
    if (rc != MML_OK) return rc;
    const int nprob = count / window;
    double* hx = stage_alloc(ctx, 6 * (size_t)count + 8 * (size_t)nprob);  // pinned read-back area: poses, then summaries
    double* hs = hx + 6 * (size_t)count;
    MML_HIP(hipMemcpyAsync(hx, ctx->d_x + 6 * (size_t)first_slot, sizeof(double) * 6 * count, hipMemcpyDeviceToHost,
                           MML_STREAM(ctx)));
    MML_HIP(hipMemcpyAsync(hs, ctx->d_summ + 8 * (size_t)first_slot, sizeof(double) * 8 * (size_t)nprob, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    if (trace)
        MML_HIP(hipMemcpyAsync(trace, ctx->d_trace + (size_t)first_slot * 6 * 64, sizeof(double) * (size_t)nprob * opts->max_num_iterations * 6 * window,
                               hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    if (window > 1 && !trace) {  // frame-parallel path: the first chunk of rounds ran; go on where a problem has not stopped
        bool open = false;
        for (int p = 0; p < nprob; ++p) open = open || hs[8 * p + 5] != 0.0;
        if (open) {
            rc = mml_window_solve_continue(ctx, first_slot, count, window, d_Tbl, *opts);
            if (rc != MML_OK) return rc;
            MML_HIP(hipMemcpyAsync(hx, ctx->d_x + 6 * (size_t)first_slot, sizeof(double) * 6 * count, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
            MML_HIP(hipMemcpyAsync(hs, ctx->d_summ + 8 * (size_t)first_slot, sizeof(double) * 8 * (size_t)nprob, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
            MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
        }
    }
    memcpy(x, hx, sizeof(double) * 6 * count);
    if (summaries)
        for (int p = 0; p < nprob; ++p) {
            summaries[p].iterations = (int)hs[8 * p];
            summaries[p].successful = (int)hs[8 * p + 1];
            summaries[p].initial_cost = hs[8 * p + 2];
            summaries[p].final_cost = hs[8 * p + 3];
            summaries[p].termination = (int)hs[8 * p + 4];
        }
    return MML_OK;
}

// ---- small host-side SO(3) helpers for the orchestration entry points (outside the kernels) ----------------
// (not imu_math.h's so3_exp_q / so3_log: these call libm where those call mml_sin / mml_cos / mml_atan, and pinned results depend on it)
static void so3_exp_h(const double* phi, double* q) {  // sophus/so3.hpp:585-622
    double th2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2];
    double imag, real;
    if (th2 < 1e-20) {
        double th4 = th2 * th2;
        imag = 0.5 - (1.0 / 48.0) * th2 + (1.0 / 3840.0) * th4;
        real = 1.0 - (1.0 / 8.0) * th2 + (1.0 / 384.0) * th4;
    } else {
        double th = sqrt(th2), half = 0.5 * th;
        imag = sin(half) / th;
        real = cos(half);
    }
    q[0] = imag * phi[0];
    q[1] = imag * phi[1];
    q[2] = imag * phi[2];
    q[3] = real;
}
static void so3_log_h(const double* qin, double* phi) {  // sophus/so3.hpp:247-287
    double nq = sqrt((qin[0] * qin[0] + qin[2] * qin[2]) + (qin[1] * qin[1] + qin[3] * qin[3]));
    double q[4] = {qin[0] / nq, qin[1] / nq, qin[2] / nq, qin[3] / nq};
    double sn = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    double w = q[3], f;
    if (sn < 1e-20) {
        f = 2.0 / w - (2.0 / 3.0) * sn / (w * w * w);
    } else {
        double n = sqrt(sn);
        if (fabs(w) < 1e-10)
            f = (w > 0 ? M_PI : -M_PI) / n;
        else
            f = 2.0 * atan(n / w) / n;
    }
    phi[0] = f * q[0];
    phi[1] = f * q[1];
    phi[2] = f * q[2];
}
// T_bl = inverse(exTlb) (Estimator.cpp:157-159 / :1155-1156)
static void invert_extrinsic(const double* exTlb, double* T_bl) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T_bl[4 * r + c] = exTlb[4 * c + r];
    for (int r = 0; r < 3; ++r)
        T_bl[4 * r + 3] = -1.0 * ((T_bl[4 * r] * exTlb[3] + T_bl[4 * r + 1] * exTlb[7]) + T_bl[4 * r + 2] * exTlb[11]);
    T_bl[12] = T_bl[13] = T_bl[14] = 0;
    T_bl[15] = 1;
}
// transformTobeMapped = [Q * exRbl, Q * exPbl + P] (Estimator.cpp:1268-1270) from x = [t, phi]
static void pose_to_Twl(const double* q, const double* P, const double* T_bl, double* T) {
    const M3 Rq = quat_to_m3(q);
    const double* R = Rq.a;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
            T[4 * r + c] = (R[3 * r] * T_bl[c] + R[3 * r + 1] * T_bl[4 + c]) + R[3 * r + 2] * T_bl[8 + c];
        T[4 * r + 3] = ((R[3 * r] * T_bl[3] + R[3 * r + 1] * T_bl[7]) + R[3 * r + 2] * T_bl[11]) + P[r];
    }
    T[12] = T[13] = T[14] = 0;
    T[15] = 1;
}

// ---- the pose calls (mml_step, mml_estimate): one parameter block down, one read-back up --------------------
// Fills the pinned twin of `dev` (returned in *host) and sends it down in ONE copy on the current lane.  dR / dt null: a call
// without sweep motions, the copy starts behind their field.  Q null: the association poses come from x, else from Q as it is.
static int pose_upload(mml_ctx* ctx, const PoseBlock& dev, const double* dR, const double* dt, const double* x, const double* Q,
                       const double* T_bl, PoseBlock* host) {
    const PoseBlock h = dev.at(stage_alloc(ctx, dev.size()));
    for (size_t i = 0; i < (size_t)dev.count; ++i) {
        if (dR) {
            memcpy(h.und() + PoseBlock::kUnd * i, dR + 9 * i, sizeof(double) * 9);
            memcpy(h.und() + PoseBlock::kUnd * i + 9, dt + 3 * i, sizeof(double) * 3);
        }
        double q[4];
        if (!Q) so3_exp_h(x + 6 * i + 3, q);
        pose_to_Twl(Q ? Q + 4 * i : q, x + 6 * i, T_bl, h.T_wl() + PoseBlock::kTwl * i);
    }
    memcpy(h.x(), x, sizeof(double) * PoseBlock::kX * dev.count);
    memcpy(h.T_bl(), T_bl, sizeof(double) * PoseBlock::kTbl);
    const size_t from = dR ? dev.o_und() : dev.o_Twl();
    MML_HIP(hipMemcpyAsync(dev.base + from, h.base + from, sizeof(double) * (dev.size() - from), hipMemcpyHostToDevice, MML_STREAM(ctx)));
    *host = h;
    return MML_OK;
}

// The pinned read-back area of a call of `count` slots from `first`, MML_SOLVE_RESULT doubles per slot.  packed: k_solve's result
// records.  Else: the poses from d_x (6 per slot) | the two ft_n rows (ints) | with `stats` the association statistics (16 per slot).
struct PoseBack {
    bool packed, stats;
    int first, count;
    double* h;
    int* ftn() const { return reinterpret_cast<int*>(h + 6 * (size_t)count); }
    double* stat() const { return h + 7 * (size_t)count; }
};
static_assert(6 + 1 + 16 <= MML_SOLVE_RESULT, "the unpacked read-back fits the area of the records");

// the solve of one block on the current lane and its part of the read-back behind it
static int pose_solve_enqueue(mml_ctx* ctx, const PoseBlock& dev, const PoseBlock& host, const mml_solve_opts& so, const PoseBack& back) {
    const int f = dev.first;
    const size_t c = (size_t)dev.count, off = (size_t)(f - back.first);
    if (back.packed) {
        double* d_res = ctx->d_result + MML_SOLVE_RESULT * (size_t)f;
        int rc = mml_launch_solve(ctx, f, dev.count, 1, dev.T_bl(), so, false, dev.x(), d_res);
        if (rc != MML_OK) return rc;
        MML_HIP(hipMemcpyAsync(back.h + MML_SOLVE_RESULT * off, d_res, sizeof(double) * MML_SOLVE_RESULT * c, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
        return MML_OK;
    }
    // (without result records k_solve starts from d_x and leaves the poses there)
    MML_HIP(hipMemcpyAsync(ctx->d_x + 6 * (size_t)f, host.x(), sizeof(double) * 6 * c, hipMemcpyHostToDevice, MML_STREAM(ctx)));
    int rc = mml_launch_solve(ctx, f, dev.count, 1, dev.T_bl(), so, false);
    if (rc != MML_OK) return rc;
    MML_HIP(hipMemcpyAsync(back.h + 6 * off, ctx->d_x + 6 * (size_t)f, sizeof(double) * 6 * c, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    for (int kind = 0; kind < 2; ++kind)
        MML_HIP(hipMemcpyAsync(back.ftn() + (size_t)kind * back.count + off, ctx->ft_n + (size_t)kind * ctx->B + f, sizeof(int) * c,
                               hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    if (back.stats)
        MML_HIP(hipMemcpyAsync(back.stat() + 16 * off, ctx->assoc_stats + 16 * (size_t)f, sizeof(double) * 16 * c, hipMemcpyDeviceToHost,
                               MML_STREAM(ctx)));
    return MML_OK;
}

// after the synchronisation: the poses (6 per slot), the stack sizes (ftn[kind * count + i]; a negative one is the down-sampler's
// overflow mark) and, for a read-back with statistics, those
static void pose_back_finish(const PoseBack& b, double* x, int* ftn, mml_assoc_stats* st) {
    const size_t n = (size_t)b.count;
    if (!b.packed) {
        memcpy(x, b.h, sizeof(double) * 6 * n);
        memcpy(ftn, b.ftn(), sizeof(int) * 2 * n);
    }
    for (size_t i = 0; i < n; ++i) {
        const double* r = b.h + MML_SOLVE_RESULT * i;  // the record: pose (6), the two stack sizes, association statistics (16)
        if (b.packed) {
            memcpy(x + 6 * i, r, sizeof(double) * 6);
            ftn[i] = (int)r[6];
            ftn[n + i] = (int)r[7];
        }
        if (st) finish_stats(b.packed ? r + 8 : b.stat() + 16 * i, &st[i]);
    }
}

// Estimator::Estimate's outer loop and convergence test for `count` slots (mml_estimate, mml_world_map_localize): the start poses
// down, the association of outer iteration `it` -- against the local maps with the 25 -> 10 -> 1 schedule, or, wm != NULL, against
// the surfel world map with wm[min(it, 2)] --, the solve behind it, ONE read-back and host synchronisation per outer iteration.
static int estimate_loop(mml_ctx* ctx, int first_slot, int count, const double* exTlb, double* P, double* Q, int max_outer, int inner_iters,
                         mml_estimate_info* info, const mml_wm_assoc_opts* wm) {
    double T_bl[16];
    invert_extrinsic(exTlb, T_bl);
    std::vector<int> done(count, 0), outer(count, 0), degen(count, 0);
    std::vector<double> x(6 * (size_t)count), xs(6 * (size_t)count);
    std::vector<mml_assoc_stats> st(count);
    std::vector<int> fn(2 * (size_t)count, 0);  // the slots' stack sizes as the last read-back reported them
    const bool packed = mml_pose_packed(count, ctx->cus);
    const PoseBlock dev = PoseBlock::of(ctx->d_pose_in, first_slot, count);
    mml_solve_opts so;
    so.max_num_iterations = inner_iters;
    so.fixed_iterations = 0;
    so.huber_delta = 0.1 / 1.5e-3;  // :1221
    so.plan_weight_tan = 0.0;       // :1206
    for (int it = 0; it < max_outer; ++it) {
        bool any = false;
        for (int i = 0; i < count; ++i)
            if (!done[i]) any = true;
        if (!any) break;
        for (int i = 0; i < count; ++i) {
            so3_log_h(Q + 4 * i, &x[6 * i + 3]);  // vector2double :937-950
            x[6 * i] = P[3 * i];
            x[6 * i + 1] = P[3 * i + 1];
            x[6 * i + 2] = P[3 * i + 2];
        }
        // association and solve are enqueued back to back and read back together: one host synchronisation per outer
        // iteration (the statistics of the association only feed the degeneracy flag, nothing the solve waits for)
        PoseBlock host;
        int rc = pose_upload(ctx, dev, nullptr, nullptr, x.data(), Q, T_bl, &host);
        if (rc != MML_OK) return rc;
        if (wm) {
            rc = mml_launch_wm_associate(ctx, first_slot, count, dev.T_wl(), wm[it < 2 ? it : 2]);
            if (rc == MML_OK) rc = mml_ensure_assoc_stats(ctx, first_slot, count);
        } else {
            const double thres = it == 0 ? 25.0 : (it == 1 ? 10.0 : 1.0);  // Estimator.cpp:1207, :1377-1381
            rc = mml_launch_associate(ctx, first_slot, count, dev.T_wl(), thres, true);
        }
        if (rc != MML_OK) return rc;
        const PoseBack back{packed, true, first_slot, count, stage_alloc(ctx, MML_SOLVE_RESULT * (size_t)count)};
        rc = pose_solve_enqueue(ctx, dev, host, so, back);
        if (rc != MML_OK) return rc;
        MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
        pose_back_finish(back, xs.data(), fn.data(), st.data());
        for (int i = 0; i < count; ++i) {
            if (done[i]) continue;
            if (st[i].is_degenerate) degen[i] = 1;
            double qa[4];
            so3_exp_h(&xs[6 * i + 3], qa);  // double2vector :952-964
            const double* qb = Q + 4 * i;
            // angularDistance (:1444): d = qb * conj(qa); 2 atan2(|d.vec|, |d.w|)
            double cx = -qa[0], cy = -qa[1], cz = -qa[2], cw = qa[3];
            double dx = qb[3] * cx + qb[0] * cw + qb[1] * cz - qb[2] * cy;
            double dy = qb[3] * cy + qb[1] * cw + qb[2] * cx - qb[0] * cz;
            double dz = qb[3] * cz + qb[2] * cw + qb[0] * cy - qb[1] * cx;
            double dw = qb[3] * cw - qb[0] * cx - qb[1] * cy - qb[2] * cz;
            double deltaR = (2.0 * atan2(sqrt((dx * dx + dy * dy) + dz * dz), fabs(dw))) * 180.0 / M_PI;
            double ex = P[3 * i] - xs[6 * i], ey = P[3 * i + 1] - xs[6 * i + 1], ez = P[3 * i + 2] - xs[6 * i + 2];
            double deltaT = sqrt((ex * ex + ey * ey) + ez * ez);
            for (int c = 0; c < 3; ++c) P[3 * i + c] = xs[6 * i + c];
            for (int c = 0; c < 4; ++c) Q[4 * i + c] = qa[c];
            outer[i] = it + 1;
            if ((deltaR < 0.05 && deltaT < 0.05) || (it + 1) == max_outer) done[i] = 1;  // :1448
        }
    }
    if (info)
        for (int i = 0; i < count; ++i) {
            info[i].outer_iterations = outer[i];
            info[i].is_degenerate = degen[i];
            info[i].n_corner_feat = fn[i];
            info[i].n_surf_feat = fn[count + i];
        }
    return MML_OK;
}

int mml_estimate(mml_ctx* ctx, int first_slot, int count, const double* exTlb, double* P, double* Q, int max_outer,
                 int inner_iters, mml_estimate_info* info) {
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(exTlb && P && Q && max_outer >= 1 && inner_iters >= 0, MML_ERR_INVALID, "bad arguments");
    {
        const int ready = mml_assoc_ready(ctx, first_slot, count, "mml_estimate");
        if (ready != MML_OK) return ready;
    }
    return estimate_loop(ctx, first_slot, count, exTlb, P, Q, max_outer, inner_iters, info, nullptr);
}

// ---- localisation in a surfel world map (world_map_assoc.hip): the entry points beside the calls they mirror ----
int mml_world_map_associate(mml_ctx* ctx, int first_slot, int count, const int* map_of_slot, const double* T_wl,
                            const mml_wm_assoc_opts* opts, mml_assoc_stats* stats) {
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(T_wl != nullptr, MML_ERR_INVALID, "mml_world_map_associate: null T_wl");
    int rc = mml_wm_assoc_ready(ctx, "mml_world_map_associate", first_slot, count, map_of_slot, opts, false);
    if (rc != MML_OK) return rc;
    double* d_T = ctx->d_pose_in + kPoseSlotDoubles * (size_t)first_slot;
    rc = upload_doubles(ctx, d_T, T_wl, 16 * (size_t)count);
    if (rc != MML_OK) return rc;
    rc = mml_launch_wm_associate(ctx, first_slot, count, d_T, *opts);
    if (rc != MML_OK || !stats) return rc;
    rc = mml_ensure_assoc_stats(ctx, first_slot, count);
    if (rc != MML_OK) return rc;
    double* h = stage_alloc(ctx, 16 * (size_t)count);  // pinned
    MML_HIP(hipMemcpyAsync(h, ctx->assoc_stats + 16 * (size_t)first_slot, sizeof(double) * 16 * (size_t)count, hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    for (int i = 0; i < count; ++i) {  // (a slot that was skipped: zeros)
        if (map_of_slot[i] < 0)
            memset(&stats[i], 0, sizeof(stats[i]));
        else
            finish_stats(h + 16 * i, &stats[i]);
    }
    return MML_OK;
}

int mml_world_map_localize(mml_ctx* ctx, int first_slot, int count, const int* map_of_slot, const double* exTlb, double* P, double* Q,
                           const mml_wm_localize_opts* opts, mml_estimate_info* info) {
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(exTlb && P && Q && opts, MML_ERR_INVALID, "mml_world_map_localize: null exTlb / P / Q / opts");
    MML_REQUIRE(opts->max_outer >= 1 && opts->inner_iters >= 0, MML_ERR_INVALID, "mml_world_map_localize: max_outer < 1 or inner_iters < 0");
    mml_wm_assoc_opts ao[3];
    for (int k = 0; k < 3; ++k) {
        ao[k] = opts->assoc;
        ao[k].max_plane_dist = opts->max_plane_dist_by_outer[k];
        if (!isfinite(ao[k].max_plane_dist) || ao[k].max_plane_dist < 0.0)
            return mml_refuse(ctx, MML_ERR_INVALID, "mml_world_map_localize: max_plane_dist_by_outer[%d] must be finite and >= 0", k);
    }
    const int rc = mml_wm_assoc_ready(ctx, "mml_world_map_localize", first_slot, count, map_of_slot, &ao[0], true);
    if (rc != MML_OK) return rc;
    return estimate_loop(ctx, first_slot, count, exTlb, P, Q, opts->max_outer, opts->inner_iters, info, ao);
}

// ---- relocalisation in a surfel world map (world_map_score.hip): the score call, the search grid and the search ----
int mml_world_map_score(mml_ctx* ctx, int first_slot, int count, const int* map_of_slot, int n_hyp, const double* T_wl,
                        const mml_wm_score_opts* opts, mml_wm_score* out) {
    CHECK_SLOTS(first_slot, count);
    return mml_wm_score_run(ctx, "mml_world_map_score", first_slot, count, map_of_slot, n_hyp, T_wl, opts, out, true);
}

// The shape of mml_wm_pose_grid: k steps on each side of an axis, floor(half / step) with 1e-9 added to the quotient, so that
// 0.6 / 0.2 counts three; nw: the yaw cells, one fewer than 2 kw + 1 when they cover the circle.  Plain host arithmetic.
struct WmGridShape {
    long kx, kz, kw, nx, nz, nw, n;
    bool cyclic;
};
static bool wm_grid_axis(double half, double step, long& k) {
    k = 0;
    if (!isfinite(half) || !isfinite(step) || half < 0.0) return false;
    if (half == 0.0) return true;
    if (!(step > 0.0)) return false;
    const double q = floor(half / step + 1e-9);
    if (!(q <= (double)(1 << 22))) return false;
    k = (long)q;
    return true;
}
static bool wm_grid_shape(double half_xy, double step_xy, double half_z, double step_z, double half_yaw, double step_yaw, WmGridShape& g) {
    if (!wm_grid_axis(half_xy, step_xy, g.kx) || !wm_grid_axis(half_z, step_z, g.kz) || !wm_grid_axis(half_yaw, step_yaw, g.kw)) return false;
    if (half_yaw > M_PI) return false;
    g.nx = 2 * g.kx + 1;
    g.nz = 2 * g.kz + 1;
    g.nw = 2 * g.kw + 1;
    g.cyclic = g.kw > 0 && fabs(2.0 * (double)g.kw * step_yaw - 2.0 * M_PI) <= 1e-9;
    if (g.cyclic) g.nw -= 1;  // (the last cell would repeat the first)
    if (((double)g.nx * (double)g.nx) * ((double)g.nz * (double)g.nw) > (double)(1 << 22)) return false;
    g.n = g.nx * g.nx * g.nz * g.nw;
    return true;
}

int mml_wm_pose_grid(const double* seed, double half_xy, double step_xy, double half_z, double step_z, double half_yaw, double step_yaw,
                     double* out, long capacity, long* n_hyp) {
    if (!seed || !n_hyp) return MML_ERR_INVALID;
    for (int c = 0; c < 12; ++c)
        if (!isfinite(seed[c])) return MML_ERR_INVALID;
    WmGridShape g;
    if (!wm_grid_shape(half_xy, step_xy, half_z, step_z, half_yaw, step_yaw, g)) return MML_ERR_INVALID;
    *n_hyp = g.n;
    if (!out) return MML_OK;
    if (capacity < g.n) return MML_ERR_CAPACITY;
    for (long iw = 0; iw < g.nw; ++iw) {
        const double yaw = (double)(iw - g.kw) * step_yaw, cw = cos(yaw), sw = sin(yaw);
        for (long iz = 0; iz < g.nz; ++iz)
            for (long iy = 0; iy < g.nx; ++iy)
                for (long ix = 0; ix < g.nx; ++ix) {
                    double* T = out + 16 * (((iw * g.nz + iz) * g.nx + iy) * g.nx + ix);
                    for (int c = 0; c < 3; ++c) {  // Rz(yaw) R_seed
                        T[c] = cw * seed[c] - sw * seed[4 + c];
                        T[4 + c] = sw * seed[c] + cw * seed[4 + c];
                        T[8 + c] = seed[8 + c];
                    }
                    T[3] = seed[3] + (double)(ix - g.kx) * step_xy;
                    T[7] = seed[7] + (double)(iy - g.kx) * step_xy;
                    T[11] = seed[11] + (double)(iz - g.kz) * step_z;
                    T[12] = T[13] = T[14] = 0.0;
                    T[15] = 1.0;
                }
    }
    return MML_OK;
}

// [Q, P] = T_wl exTlb: the inverse of pose_to_Twl (T_wl = [Q, P] inverse(exTlb))
int mml_wm_body_pose(const double* T_wl, const double* exTlb, double* P, double* Q) {
    if (!T_wl || !exTlb || !P || !Q) return MML_ERR_INVALID;
    M3 R;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R.a[3 * r + c] = (T_wl[4 * r] * exTlb[c] + T_wl[4 * r + 1] * exTlb[4 + c]) + T_wl[4 * r + 2] * exTlb[8 + c];
        P[r] = ((T_wl[4 * r] * exTlb[3] + T_wl[4 * r + 1] * exTlb[7]) + T_wl[4 * r + 2] * exTlb[11]) + T_wl[4 * r + 3];
    }
    double q[4];
    m3_to_quat(R, q);
    const double n = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    for (int c = 0; c < 4; ++c) Q[c] = q[c] / n;
    return MML_OK;
}

// T_wl = [Q, P] inverse(exTlb), as estimate_loop composes it
int mml_wm_lidar_pose(const double* P, const double* Q, const double* exTlb, double* T_wl) {
    if (!P || !Q || !exTlb || !T_wl) return MML_ERR_INVALID;
    double T_bl[16];
    invert_extrinsic(exTlb, T_bl);
    pose_to_Twl(Q, P, T_bl, T_wl);
    return MML_OK;
}

void mml_wm_reloc_opts_default(mml_wm_reloc_opts* o, float leaf) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->half_xy = 2.0;
    o->step_xy = 0.5;
    o->half_z = 0.0;
    o->step_z = 0.5;
    o->half_yaw = M_PI;
    o->step_yaw = M_PI / 16.0;
    o->levels = 2;
    o->refine = 2;
    o->keep = 4;
    mml_wm_score_opts_default(&o->score, leaf);
    mml_wm_localize_opts_default(&o->localize, leaf);
}

int mml_world_map_relocalize(mml_ctx* ctx, int first_slot, int count, const int* map_of_slot, const double* exTlb, double* P, double* Q,
                             const mml_wm_reloc_opts* o, mml_wm_reloc_info* info) {
    static const char* who = "mml_world_map_relocalize";
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(exTlb && P && Q && o, MML_ERR_INVALID, "mml_world_map_relocalize: null exTlb / P / Q / opts");
    if (o->levels < 1 || o->levels > 3) return mml_refuse(ctx, MML_ERR_INVALID, "%s: levels %d outside 1..3", who, o->levels);
    if (o->refine < 2 || o->refine > 4) return mml_refuse(ctx, MML_ERR_INVALID, "%s: refine %d outside 2..4", who, o->refine);
    if (o->keep < 1 || o->keep > 16) return mml_refuse(ctx, MML_ERR_INVALID, "%s: keep %d outside 1..16", who, o->keep);
    if (o->score.stride < 1) return mml_refuse(ctx, MML_ERR_INVALID, "%s: stride %d < 1", who, o->score.stride);
    if (!(isfinite(o->score.assoc.max_plane_dist) && o->score.assoc.max_plane_dist > 0.0))
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: score.assoc.max_plane_dist must be finite and > 0 (the score divides by it)", who);
    MML_REQUIRE(o->localize.max_outer >= 1 && o->localize.inner_iters >= 0, MML_ERR_INVALID, "mml_world_map_relocalize: localize.max_outer < 1 or inner_iters < 0");
    for (int k = 0; k < 3; ++k) {
        mml_wm_assoc_opts a = o->localize.assoc;
        a.max_plane_dist = o->localize.max_plane_dist_by_outer[k];
        const int rc = mml_wm_assoc_opts_ok(ctx, who, &a);
        if (rc != MML_OK) return rc;
    }
    for (int i = 0; i < count; ++i)
        for (int c = 0; c < 7; ++c)
            if (!isfinite(c < 3 ? P[3 * i + c] : Q[4 * i + c - 3])) return mml_refuse(ctx, MML_ERR_INVALID, "%s: the seed pose of slot %d is not finite", who, first_slot + i);
    for (int c = 0; c < 12; ++c)
        if (!isfinite(exTlb[c])) return mml_refuse(ctx, MML_ERR_INVALID, "%s: exTlb is not finite", who);
    // the shapes of all levels, before anything runs: level l > 0 holds, per kept hypothesis, the grid of +-1 step of level l - 1
    WmGridShape shape[3];
    double step[3][3];  // per level: xy, z, yaw
    long kept[3], n_level[3];
    for (int l = 0; l < o->levels; ++l) {
        bool ok;
        if (l == 0) {
            step[0][0] = o->step_xy, step[0][1] = o->step_z, step[0][2] = o->step_yaw;
            ok = wm_grid_shape(o->half_xy, o->step_xy, o->half_z, o->step_z, o->half_yaw, o->step_yaw, shape[0]);
            kept[0] = 1;
        } else {
            for (int a = 0; a < 3; ++a) step[l][a] = step[l - 1][a] / (double)o->refine;
            const WmGridShape& p = shape[l - 1];  // (an axis of one cell stays one cell)
            ok = wm_grid_shape(p.kx ? step[l - 1][0] : 0.0, step[l][0], p.kz ? step[l - 1][1] : 0.0, step[l][1], p.kw ? step[l - 1][2] : 0.0, step[l][2], shape[l]);
            kept[l] = n_level[l - 1] < o->keep ? n_level[l - 1] : o->keep;
        }
        if (!ok) return mml_refuse(ctx, MML_ERR_INVALID, "%s: mml_wm_pose_grid refuses the grid of level %d (not finite, half < 0, half_yaw > pi, step <= 0 or above 2^22 cells)", who, l);
        n_level[l] = kept[l] * shape[l].n;
        if (n_level[l] > 65536 || (long long)count * n_level[l] > (1LL << 22))
            return mml_refuse(ctx, MML_ERR_INVALID, "%s: level %d has %ld hypotheses per slot: above 65536, or above 2^22 for the %d slots", who, l, n_level[l], count);
    }
    int rc = mml_wm_assoc_ready(ctx, who, first_slot, count, map_of_slot, &o->score.assoc, true);
    if (rc != MML_OK) return rc;
    double T_bl[16];
    invert_extrinsic(exTlb, T_bl);
    std::vector<double> T, Tprev;
    std::vector<mml_wm_score> sc;
    std::vector<mml_wm_reloc_info> inf((size_t)count);
    memset(static_cast<void*>(inf.data()), 0, sizeof(mml_wm_reloc_info) * (size_t)count);
    std::vector<long> top((size_t)count * 16, 0);  // per slot: the kept hypotheses of the level, best first
    for (int l = 0; l < o->levels; ++l) {
        const size_t H = (size_t)n_level[l];
        T.assign(16 * H * (size_t)count, 0.0);
        for (int i = 0; i < count; ++i)
            for (long k = 0; k < kept[l]; ++k) {
                double seed[16];
                if (l == 0)
                    pose_to_Twl(Q + 4 * i, P + 3 * i, T_bl, seed);
                else
                    memcpy(seed, &Tprev[16 * ((size_t)i * (size_t)n_level[l - 1] + (size_t)top[16 * (size_t)i + (size_t)k])], sizeof(seed));
                const WmGridShape& p = shape[l > 0 ? l - 1 : 0];
                long n = 0;
                rc = l == 0 ? mml_wm_pose_grid(seed, o->half_xy, o->step_xy, o->half_z, o->step_z, o->half_yaw, o->step_yaw, &T[16 * H * (size_t)i], (long)H, &n)
                            : mml_wm_pose_grid(seed, p.kx ? step[l - 1][0] : 0.0, step[l][0], p.kz ? step[l - 1][1] : 0.0, step[l][1],
                                               p.kw ? step[l - 1][2] : 0.0, step[l][2], &T[16 * (H * (size_t)i + (size_t)(k * shape[l].n))], shape[l].n, &n);
                if (rc != MML_OK || n != shape[l].n) return mml_refuse(ctx, MML_ERR_INVALID, "%s: the grid of level %d around slot %d could not be made", who, l, first_slot + i);
            }
        sc.assign(H * (size_t)count, mml_wm_score{0, 0, 0});
        rc = mml_wm_score_run(ctx, who, first_slot, count, map_of_slot, (int)H, T.data(), &o->score, sc.data(), false);
        if (rc != MML_OK) return rc;
        const long keep_n = (long)H < o->keep ? (long)H : o->keep;
        for (int i = 0; i < count; ++i) {
            const mml_wm_score* s = &sc[H * (size_t)i];
            long* tp = &top[16 * (size_t)i];
            for (long k = 0; k < keep_n; ++k) {  // selection of the keep_n best, in ranking order
                long b = -1;
                for (long h = 0; h < (long)H; ++h) {
                    bool taken = false;
                    for (long j = 0; j < k; ++j) taken = taken || tp[j] == h;
                    if (taken) continue;
                    if (b < 0 || mml_wms_better(s[h].score_q, s[h].n_match, h, s[b].score_q, s[b].n_match, b)) b = h;
                }
                tp[k] = b;
            }
            inf[(size_t)i].n_hyp_scored += (long)H;
            if (l == 0) {
                const WmGridShape& g = shape[0];
                inf[(size_t)i].best = s[tp[0]];
                const long b = tp[0], bx = b % g.nx, by = (b / g.nx) % g.nx, bz = (b / (g.nx * g.nx)) % g.nz, bw = b / (g.nx * g.nx * g.nz);
                long second = -1;
                for (long h = 0; h < (long)H; ++h) {
                    const long hx = h % g.nx, hy = (h / g.nx) % g.nx, hz = (h / (g.nx * g.nx)) % g.nz, hw = h / (g.nx * g.nx * g.nz);
                    long dw = labs(hw - bw);
                    if (g.cyclic && g.nw - dw < dw) dw = g.nw - dw;
                    if (labs(hx - bx) <= 1 && labs(hy - by) <= 1 && labs(hz - bz) <= 1 && dw <= 1) continue;  // a neighbour (or the best itself)
                    if (second < 0 || mml_wms_better(s[h].score_q, s[h].n_match, h, s[second].score_q, s[second].n_match, second)) second = h;
                }
                if (second >= 0) inf[(size_t)i].second = s[second];
            }
            if (l == o->levels - 1) memcpy(inf[(size_t)i].T_start, &T[16 * (H * (size_t)i + (size_t)tp[0])], sizeof(double) * 16);
        }
        Tprev.swap(T);
    }
    std::vector<double> Ps(3 * (size_t)count), Qs(4 * (size_t)count);
    for (int i = 0; i < count; ++i) mml_wm_body_pose(inf[(size_t)i].T_start, exTlb, &Ps[3 * (size_t)i], &Qs[4 * (size_t)i]);
    std::vector<mml_estimate_info> est((size_t)count);
    rc = mml_world_map_localize(ctx, first_slot, count, map_of_slot, exTlb, Ps.data(), Qs.data(), &o->localize, est.data());
    if (rc != MML_OK) return rc;
    T.assign(16 * (size_t)count, 0.0);
    for (int i = 0; i < count; ++i) pose_to_Twl(&Qs[4 * (size_t)i], &Ps[3 * (size_t)i], T_bl, &T[16 * (size_t)i]);
    sc.assign((size_t)count, mml_wm_score{0, 0, 0});
    rc = mml_wm_score_run(ctx, who, first_slot, count, map_of_slot, 1, T.data(), &o->score, sc.data(), false);
    if (rc != MML_OK) return rc;
    memcpy(P, Ps.data(), sizeof(double) * 3 * (size_t)count);
    memcpy(Q, Qs.data(), sizeof(double) * 4 * (size_t)count);
    if (info)
        for (int i = 0; i < count; ++i) {
            inf[(size_t)i].final = sc[(size_t)i];
            inf[(size_t)i].est = est[(size_t)i];
            info[i] = inf[(size_t)i];
        }
    return MML_OK;
}

int mml_step(mml_ctx* ctx, int first_slot, int count, const double* dR, const double* dt, const double* exTlb,
             double thres_dist, int gn_iters, double* x_inout) {
    CHECK_SLOTS(first_slot, count);
    MML_REQUIRE(dR && dt && exTlb && x_inout, MML_ERR_INVALID, "null argument");
    MML_REQUIRE(gn_iters >= 0 && gn_iters <= 64, MML_ERR_INVALID, "gn_iters must be in [0, 64]");
    {
        const int ready = mml_assoc_ready(ctx, first_slot, count, "mml_step");
        if (ready != MML_OK) return ready;
    }
    double T_bl[16];
    invert_extrinsic(exTlb, T_bl);
    mml_solve_opts so;
    so.max_num_iterations = gn_iters;
    so.fixed_iterations = 1;
    so.huber_delta = 0.1 / 1.5e-3;
    so.plan_weight_tan = 0.0;
    // Sub-batches on independent streams (`lanes`, mml_set_lanes): contiguous slot ranges, each the whole chain on its own
    // stream, so that the tail of one kernel overlaps the head of another.  Scans are independent, results identical
    // (tests/test_gpu_shapes.py, bench.py replica_check).  What the lanes do NOT buy is co-residency of unlike kernels: every
    // kernel of the chain fills the CUs' registers / LDS by itself at these batch sizes.  Round 5 measured the other
    // schedule -- pieces of 512 .. 2048 scans, stream 0 extracting piece i + 1 while other streams run the back end of piece
    // i, 2 .. 5 streams, three stage-to-stream maps: 306 k .. 330 k scans/s against 355 k for two lanes (HISTORY.md).
    const int lanes = count >= 64 ? ctx->n_lanes : 1;
    const int chunk = (count + lanes - 1) / lanes;
    // Every piece has its own parameter block (pose_upload) and its part of the call's read-back.  A handful of slots (the live
    // path, `packed`) is one piece, and there every small transfer is a launch of its own in the dependency chain (a blit kernel
    // of ~4 us plus the gap in front of it): the block is the only copy down and k_solve's result records are the only copy up.
    const bool packed = mml_pose_packed(count, ctx->cus);
    const PoseBlock call = PoseBlock::of(ctx->d_pose_in, first_slot, count);
    struct Piece {
        PoseBlock dev, host;
    } pieces[mml_ctx::MAX_LANES];
    int n_pieces = 0;
    size_t need = (7 + MML_SOLVE_RESULT) * (size_t)count + 16 + 1024;  // h_x, the read-back; (the ring hands out multiples of 8)
    for (; n_pieces < lanes; ++n_pieces) {
        pieces[n_pieces].dev = call.piece(n_pieces, chunk);
        if (pieces[n_pieces].dev.count <= 0) break;
        need += pieces[n_pieces].dev.size() + 8;
    }
    // (the staging ring: a wrap in the middle of the call would drain the streams; wrap now if this call does not fit)
    if (ctx->stage_cursor + need > ctx->h_stage_doubles && need <= ctx->h_stage_doubles) {
        int rw = mml_sync_all(ctx);
        if (rw != MML_OK) return rw;
        ctx->stage_cursor = 0;
    }
    double* h_x = stage_alloc(ctx, 7 * (size_t)count + 1);  // poses, then the two stack-size arrays: what the read-back yields
    int* h_ftn = reinterpret_cast<int*>(h_x + 6 * (size_t)count);
    const PoseBack back{packed, false, first_slot, count, stage_alloc(ctx, MML_SOLVE_RESULT * (size_t)count)};
    int rc = MML_OK;
    // Entry points outside mml_step enqueue on stream 0 (mml_scan_upload's copies, a staged mml_extract ...): the other streams
    // start behind whatever stream 0 holds at this point.  (Found by running 80 slots on the default two lanes straight
    // after their uploads: the last slot's copy was still in flight when lane 1 began to bucket it.)
    if (lanes > 1) {
        if (hipEventRecord(ctx->lane_mark[0], ctx->streams[0]) != hipSuccess) return MML_ERR_HIP;
        for (int l = 1; l < mml_ctx::MAX_LANES; ++l)
            if (hipStreamWaitEvent(ctx->streams[l], ctx->lane_mark[0], 0) != hipSuccess) return MML_ERR_HIP;
    }
    auto run_stage = [&](int stage, Piece& p) -> int {
        const int f = p.dev.first, c = p.dev.count;
        const size_t off = (size_t)(f - first_slot);
        switch (stage) {
            case 0: return mml_launch_extract(ctx, f, c, false);
            case 1: {  // (the points the down-sampler reads; the rest of the cloud when somebody asks for it: mml_cloud_settle)
                int r = pose_upload(ctx, p.dev, dR + 9 * off, dt + 3 * off, x_inout + 6 * off, nullptr, T_bl, &p.host);
                if (r != MML_OK) return r;
                return ctx->lazy_undistort ? mml_launch_undistort_listed(ctx, f, c, p.dev.und()) : mml_launch_undistort(ctx, f, c, p.dev.und());
            }
            case 2: return mml_launch_downsample(ctx, f, c);
            case 3: return mml_launch_associate(ctx, f, c, p.dev.T_wl(), thres_dist, false);  // (nobody reads the statistics of a step)
            default: return pose_solve_enqueue(ctx, p.dev, p.host, so, back);
        }
    };
    // The stages are enqueued stage by stage across the lanes (each lane's stream keeps its own order): every lane has its first
    // kernels in its queue within a few tens of microseconds, instead of lane 3 waiting for the host to finish enqueueing the whole
    // chains of lanes 0..2.
    for (int stage = 0; stage < 5 && rc == MML_OK; ++stage)
        for (int l = 0; l < n_pieces && rc == MML_OK; ++l) {
            ctx->cur = l;
            rc = run_stage(stage, pieces[l]);
        }
    ctx->cur = 0;
    int rs = mml_sync_all(ctx);
    if (rc != MML_OK) return rc;
    if (rs != MML_OK) return rs;
    pose_back_finish(back, h_x, h_ftn, nullptr);
    // A negative stack size is the down-sampler's overflow mark.  Slots whose labelled cloud is merely too dense for the
    // LDS sort are redone through the global-sort filter and re-registered one by one (rare: > 8192 corner- or
    // surf-labelled points in one scan); a slot that exceeds max_features stays failed.  Either way every other slot of
    // the batch gets its pose, and a failed slot keeps the pose it came with.
    std::vector<int> bad;
    for (int i = 0; i < count; ++i)
        if (h_ftn[i] < 0 || h_ftn[count + i] < 0) bad.push_back(i);
    std::vector<char> failed((size_t)count, 0);
    for (int i : bad) {
        std::vector<int> redone;
        rc = mml_downsample_redo_overflow(ctx, first_slot + i, 1, &redone);
        bool ok = rc == MML_OK && !redone.empty();
        if (ok) {
            int fn[2] = {-1, -1};  // (on the ctx stream: the lanes are non-blocking streams, the null stream does not order with them)
            if (hipMemcpyAsync(&fn[0], ctx->ft_n + first_slot + i, sizeof(int), hipMemcpyDeviceToHost, MML_STREAM(ctx)) != hipSuccess ||
                hipMemcpyAsync(&fn[1], ctx->ft_n + ctx->B + first_slot + i, sizeof(int), hipMemcpyDeviceToHost, MML_STREAM(ctx)) != hipSuccess ||
                hipStreamSynchronize(MML_STREAM(ctx)) != hipSuccess)
                return MML_ERR_HIP;
            ok = fn[0] >= 0 && fn[1] >= 0;
        }
        if (ok) {
            double q[4], T1[16];
            so3_exp_h(x_inout + 6 * (size_t)i + 3, q);
            pose_to_Twl(q, x_inout + 6 * (size_t)i, T_bl, T1);
            rc = mml_associate(ctx, first_slot + i, 1, T1, thres_dist, nullptr);
            if (rc != MML_OK) return rc;
            double xs[6];
            memcpy(xs, x_inout + 6 * (size_t)i, sizeof(xs));
            rc = mml_solve(ctx, first_slot + i, 1, 1, T_bl, &so, xs, nullptr, nullptr);
            if (rc != MML_OK) return rc;
            memcpy(h_x + 6 * (size_t)i, xs, sizeof(xs));
        } else {
            failed[i] = 1;
        }
    }
    int n_failed = 0, first_failed = -1;
    for (int i = 0; i < count; ++i) {
        if (failed[i]) {
            if (first_failed < 0) first_failed = first_slot + i;
            ++n_failed;
            continue;
        }
        memcpy(x_inout + 6 * (size_t)i, h_x + 6 * (size_t)i, sizeof(double) * 6);
    }
    if (n_failed) {
        ctx->err = "down-sample overflowed max_features in " + std::to_string(n_failed) + " slot(s), first: slot " +
                   std::to_string(first_failed) + " (the other slots' poses were returned)";
        return MML_ERR_CAPACITY;
    }
    return MML_OK;
}

int mml_set_lanes(mml_ctx* ctx, int lanes) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(lanes >= 1 && lanes <= mml_ctx::MAX_LANES, MML_ERR_INVALID, "lanes must be in [1, 8]");
    int rc = mml_sync_all(ctx);
    if (rc != MML_OK) return rc;
    ctx->n_lanes = lanes;
    return MML_OK;
}

// ---- profiling ---------------------------------------------------------------------------------------------
int mml_profile_enable(mml_ctx* ctx, int on) {
    if (!ctx) return MML_ERR_INVALID;
    ctx->profiling = on != 0;
    return MML_OK;
}

static int drain_pending(mml_ctx* ctx) {
    int rc0 = mml_sync_all(ctx);
    if (rc0 != MML_OK) return rc0;
    for (auto& pe : ctx->pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
            ctx->stages[pe.stage].total_ms += ms;
            ctx->stages[pe.stage].launches += 1;
        }
        ctx->event_pool.push_back(pe.a);
        ctx->event_pool.push_back(pe.b);
    }
    ctx->pending.clear();
    return MML_OK;
}

int mml_profile_reset(mml_ctx* ctx) {
    if (!ctx) return MML_ERR_INVALID;
    int rc = drain_pending(ctx);
    for (auto& s : ctx->stages) {
        s.total_ms = 0;
        s.launches = 0;
    }
    return rc;
}

int mml_profile_get(mml_ctx* ctx, mml_profile* out) {
    if (!ctx || !out) return MML_ERR_INVALID;
    int rc = drain_pending(ctx);
    if (rc != MML_OK) return rc;
    out->n_stages = (int)std::min<size_t>(ctx->stages.size(), MML_MAX_STAGES);
    for (int i = 0; i < out->n_stages; ++i) {
        out->name[i] = ctx->stages[i].name.c_str();
        out->total_ms[i] = ctx->stages[i].total_ms;
        out->launches[i] = ctx->stages[i].launches;
    }
    return MML_OK;
}

int mml_extract_queue_counts(mml_ctx* ctx, int slot, int* redo, int* brk) {
    CHECK_SLOTS(slot, 1);
    int rc = mml_sync_all(ctx);
    if (rc != MML_OK) return rc;
    if (brk) MML_HIP(hipMemcpy(brk, ctx->brk_cnt + slot, sizeof(int), hipMemcpyDeviceToHost));
    if (redo) MML_HIP(hipMemcpy(redo, ctx->brk_cnt + ctx->B + slot, sizeof(int), hipMemcpyDeviceToHost));  // (redo_cnt = brk_cnt + B)
    return MML_OK;
}

int mml_associate_far_count(mml_ctx* ctx, int* n) {
    if (!ctx || !n) return MML_ERR_INVALID;
    int rc = mml_sync_all(ctx);
    if (rc != MML_OK) return rc;
    int h[mml_ctx::MAX_LANES];
    MML_HIP(hipMemcpy(h, ctx->d_misc + 32, sizeof(h), hipMemcpyDeviceToHost));  // (one counter per stream lane: map_assoc.hip hard_count)
    // (the counters of the lanes the last call did not use still hold an earlier call's counts)
    *n = 0;
    for (int l = 0; l < ctx->far_lanes; ++l) *n += h[l];
    return MML_OK;
}

int mml_device_info(mml_ctx* ctx, char* name, int name_cap, int* cus, size_t* hbm_bytes) {
    if (!ctx) return MML_ERR_INVALID;
    hipDeviceProp_t prop;
    MML_HIP(hipGetDeviceProperties(&prop, ctx->device));
    if (name && name_cap > 0) {
        strncpy(name, prop.name, name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (cus) *cus = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
    return MML_OK;
}

}  // extern "C"

namespace {
__global__ void k_copy16(const float4* __restrict__ a, float4* __restrict__ b, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) b[i] = a[i];
}
// The copy a streaming kernel of this library can actually match: 16 bytes per lane, four independent loads in flight per
// thread, non-temporal loads and stores (nothing is re-read), one workgroup per 16 KB so that the whole array is in flight on
// 8 wavefronts per SIMD (12 VGPRs).  MI355X_MICROARCH.md quotes 6.29 TB/s for a float4 copy; k_undistort sustains 5.8.
typedef float copy_v4f __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) k_copy16_nt(const copy_v4f* __restrict__ a, copy_v4f* __restrict__ b, size_t n) {
    const size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x;
    copy_v4f v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (base + 256 * r < n) v[r] = __builtin_nontemporal_load(a + base + 256 * r);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (base + 256 * r < n) __builtin_nontemporal_store(v[r], b + base + 256 * r);
}
}  // namespace

extern "C" int mml_copy_bandwidth(mml_ctx* ctx, size_t bytes, int reps, double* gbps) {
    if (!ctx || !gbps || reps <= 0) return MML_ERR_INVALID;
    MML_HIP(hipSetDevice(ctx->device));
    size_t n = bytes / 16;
    MmlTemp<float4> ta, tb;
    MML_HIP(ta.alloc(n));
    MML_HIP(tb.alloc(n));
    float4 *a = ta.d, *b = tb.d;
    MML_HIP(hipMemsetAsync(a, 1, n * 16, MML_STREAM(ctx)));
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    // two forms, the better one is reported: a grid-stride loop of plain 16-byte copies, and the non-temporal one above
    double best = 0.0;
    hipError_t e = hipSuccess;
    for (int form = 0; form < 2 && e == hipSuccess; ++form) {
        auto launch = [&]() {
            if (form == 0)
                hipLaunchKernelGGL(k_copy16, dim3(2048), dim3(256), 0, MML_STREAM(ctx), a, b, n);
            else
                hipLaunchKernelGGL(k_copy16_nt, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, MML_STREAM(ctx),
                                   reinterpret_cast<const copy_v4f*>(a), reinterpret_cast<copy_v4f*>(b), n);
        };
        launch();
        hipEventRecord(e0, MML_STREAM(ctx));
        for (int r = 0; r < reps; ++r) launch();
        hipEventRecord(e1, MML_STREAM(ctx));
        e = hipStreamSynchronize(MML_STREAM(ctx));
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && ms > 0) best = std::max(best, (2.0 * n * 16 * reps) / (ms * 1e-3) / 1e9);
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (e != hipSuccess) {
        ctx->err = hipGetErrorString(e);
        return MML_ERR_HIP;
    }
    *gbps = best;
    return MML_OK;
}

namespace {
// tools/issue_probe.hip in small: eight independent chains per lane of one instruction class, every SIMD eight wavefronts deep
template <int KIND>
__global__ __launch_bounds__(256) void k_issue_rate(float* out, float a, float b, int ia) {
    float x[8];
    int u[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        x[i] = (float)(threadIdx.x + i);
        u[i] = (int)threadIdx.x * 7 + i;
    }
    for (int it = 0; it < 2048; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if constexpr (KIND == 0) x[i] = __builtin_fmaf(x[i], a, b);
            if constexpr (KIND == 1) asm volatile("v_add_u32 %0, %0, %1" : "+v"(u[i]) : "v"(ia));
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += x[i] + (float)u[i];
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
}
}  // namespace

extern "C" int mml_issue_rate(mml_ctx* ctx, int kind, int reps, double* wave_instr_per_s) {
    if (!ctx || !wave_instr_per_s || reps <= 0 || kind < 0 || kind > 1) return MML_ERR_INVALID;
    MML_HIP(hipSetDevice(ctx->device));
    const int blocks = ctx->cus * 64;  // eight workgroups of four wavefronts per CU, eight rounds of them
    MmlTemp<float> tmp;
    MML_HIP(tmp.alloc(256 * (size_t)blocks));
    float* d = tmp.d;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    auto launch = [&]() {
        if (kind == 0)
            hipLaunchKernelGGL(k_issue_rate<0>, dim3(blocks), dim3(256), 0, MML_STREAM(ctx), d, 0.999f, 0.001f, 3);
        else
            hipLaunchKernelGGL(k_issue_rate<1>, dim3(blocks), dim3(256), 0, MML_STREAM(ctx), d, 0.999f, 0.001f, 3);
    };
    launch();
    double best = 0.0;
    hipError_t e = hipSuccess;
    for (int r = 0; r < reps && e == hipSuccess; ++r) {
        hipEventRecord(e0, MML_STREAM(ctx));
        launch();
        hipEventRecord(e1, MML_STREAM(ctx));
        e = hipStreamSynchronize(MML_STREAM(ctx));
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && ms > 0) best = std::max(best, (double)blocks * 4 * 2048 * 8 / (ms * 1e-3));
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (e != hipSuccess) {
        ctx->err = hipGetErrorString(e);
        return MML_ERR_HIP;
    }
    *wave_instr_per_s = best;
    return MML_OK;
}

// ---- the phase clocks' reader (phase_clock.h; a test hook, not in the public header) ----
namespace {
constexpr const char* kPhaseFamilies[] = {"op", "st", "sel", "sp", "vx", "sv", "svw"};
struct PhaseFamily {
    const char* name;
    const void* symbol;
    int slots;
} g_phase_built[sizeof(kPhaseFamilies) / sizeof(kPhaseFamilies[0])];  // the families this library was built with
int g_phase_nbuilt = 0;
}  // namespace
int phase_clock_register(const char* family, const void* symbol, int slots) {
    g_phase_built[g_phase_nbuilt++] = {family, symbol, slots};
    return 0;
}
// reset != 0: zeroes the family's slots; else copies them to out[capacity].  Returns the slot count, -1 for a name that is no family,
// -2 for a family this library was not built with (both before any HIP call), -3 for an out that is missing or too small, -4 HIP error
extern "C" int mml_debug_phase_clocks(const char* family, unsigned long long* out, int capacity, int reset) {
    bool known = false;
    for (const char* name : kPhaseFamilies) known = known || (family && !strcmp(family, name));
    if (!known) return -1;
    const PhaseFamily* f = nullptr;
    for (int i = 0; i < g_phase_nbuilt; ++i)
        if (!strcmp(family, g_phase_built[i].name)) f = &g_phase_built[i];
    if (!f) return -2;
    const size_t bytes = sizeof(unsigned long long) * f->slots;
    if (reset) {
        const unsigned long long zeros[PHASE_CLOCK_MAX_SLOTS] = {};
        return hipMemcpyToSymbol(f->symbol, zeros, bytes) == hipSuccess ? f->slots : -4;
    }
    if (!out || capacity < f->slots) return -3;
    return hipMemcpyFromSymbol(out, f->symbol, bytes) == hipSuccess ? f->slots : -4;
}

int mml_stage_begin(mml_ctx* ctx, const char* name) {
    if (!ctx->profiling) return -1;
    int idx = -1;
    for (size_t i = 0; i < ctx->stages.size(); ++i)
        if (ctx->stages[i].name == name) idx = (int)i;
    if (idx < 0) {
        MmlStageTimer t;
        t.name = name;
        ctx->stages.push_back(t);
        idx = (int)ctx->stages.size() - 1;
    }
    mml_ctx::Pending pe;
    pe.stage = idx;
    auto get = [&]() {
        hipEvent_t e;
        if (!ctx->event_pool.empty()) {
            e = ctx->event_pool.back();
            ctx->event_pool.pop_back();
        } else {
            hipEventCreate(&e);
        }
        return e;
    };
    pe.a = get();
    pe.b = get();
    hipEventRecord(pe.a, MML_STREAM(ctx));
    ctx->pending.push_back(pe);
    return (int)ctx->pending.size() - 1;
}

void mml_stage_end(mml_ctx* ctx, int token) {
    if (token < 0) return;
    hipEventRecord(ctx->pending[token].b, MML_STREAM(ctx));
}

int mml_sync_all(mml_ctx* ctx) {
    for (int l = 0; l < mml_ctx::MAX_LANES; ++l) MML_HIP(hipStreamSynchronize(ctx->streams[l]));
    MML_HIP(hipStreamSynchronize(ctx->copy_stream));
    for (auto& u : ctx->uploads) ctx->upload_event_pool.push_back(u.done);
    ctx->uploads.clear();
    return MML_OK;
}

int mml_enter_idle(mml_ctx* ctx) {
    MML_HIP(hipSetDevice(ctx->device));
    int rc = mml_sync_all(ctx);
    if (rc != MML_OK) return rc;
    ctx->cur = 0;
    return MML_OK;
}

// Orders every lane behind the batch uploads still in flight on slots [first, first + count); finished uploads retire.
int mml_uploads_wait(mml_ctx* ctx, int first, int count) {
    for (size_t i = 0; i < ctx->uploads.size();) {
        mml_ctx::Upload& u = ctx->uploads[i];
        if (hipEventQuery(u.done) == hipSuccess) {
            ctx->upload_event_pool.push_back(u.done);
            ctx->uploads.erase(ctx->uploads.begin() + i);
            continue;
        }
        if (u.first < first + count && first < u.first + u.count)
            for (int l = 0; l < mml_ctx::MAX_LANES; ++l) MML_HIP(hipStreamWaitEvent(ctx->streams[l], u.done, 0));
        ++i;
    }
    return MML_OK;
}
