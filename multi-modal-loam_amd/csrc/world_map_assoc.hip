// world_map_assoc.hip -- association of down-sampled surf stacks against a surfel world map (mml_world_map_associate, and the
// association stage of mml_world_map_localize): plane factors from the map's surfels for `count` slots in ONE launch.  The
// arithmetic -- the feature's voxel, the candidates, the choice, the gates, the record -- is world_map_assoc.h's and nowhere
// else; the probe and the surfel record are world_map_dev.h's, the ones the add and the surfel download run.
//
// k_wm_associate  grid (max_features / 256, count), one lane per feature.  What is the same for a whole workgroup -- the slot's
//                 map, pose and the two stack sizes -- is indexed by blockIdx.y alone and comes through scalar loads, before the
//                 first store.  The up to 27 probes are wm_probe27's (world_map_dev.h, shared with k_wm_score): three groups of nine
//                 first loads, and only a probe that met another voxel's key walks on.
//                 The winner's count and moments are loaded once, one eig3_sym per lane.  The table is only read: no atomics, no
//                 LDS.  A lane below the slot's CORNER count clears the line record of its index (src = -1), so the slot is left
//                 with plane factors only, as mml_associate leaves a slot whose corner features found no model.
// The statistics are k_assoc_stats', on demand (mml_ensure_assoc_stats), exactly as after mml_associate.
#include <math.h>
#include <string.h>

#include "mml_internal.h"
#include "world_map_assoc.h"

namespace {
#include "eig3_dev.h"
#include "world_map_dev.h"

struct WaTable {
    const unsigned long long* keys;
    unsigned long long slots;
    const float4* sum;
    const int* count;
    WmMom M;
};
struct WaOpts {
    float inv;
    int nb, min_points;
    float min_planarity;
    double max_dist;
};

__global__ __launch_bounds__(256) void k_wm_associate(int first, int B, int MF, const int* __restrict__ ft_n, const float4* __restrict__ ft,
                                                      const int* __restrict__ maps, const double* __restrict__ Twl, WaTable W, WaOpts O,
                                                      MmlLineFactor* __restrict__ lf, MmlPlaneFactor* __restrict__ pf) {
    const int map = maps[blockIdx.y];
    if (map < 0) return;  // (the whole workgroup)
    const int slot = first + blockIdx.y;
    int nc = ft_n[slot], ns = ft_n[B + slot];
    nc = nc < 0 ? 0 : (nc > MF ? MF : nc);  // (the host refused a slot without a stack; an index stays inside the slot's MF)
    ns = ns < 0 ? 0 : (ns > MF ? MF : ns);
    const int b0 = blockIdx.x * blockDim.x;
    if (b0 >= nc && b0 >= ns) return;
    double T[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) T[c] = Twl[16 * (size_t)blockIdx.y + c];
    const int i = b0 + threadIdx.x;
    if (i < nc) {
        MmlLineFactor none;
        memset(&none, 0, sizeof(none));
        none.src = -1;
        lf[(size_t)slot * MF + i] = none;
    }
    if (i >= ns) return;
    const float4 f = ft[(size_t)slot * MF + i];
    float wx, wy, wz;
    mml_world_point(T, f.x, f.y, f.z, wx, wy, wz);
    int vi = 0, vj = 0, vk = 0;
    const bool ok = mml_wma_voxel(wx, wy, wz, O.inv, vi, vj, vk);
    MmlWmaBest best;
    mml_wma_best_init(best);
    if (ok) wm_probe27(W.keys, W.slots, W.sum, W.count, map, O.nb, O.min_points, vi, vj, vk, wx, wy, wz, best);
    MmlPlaneFactor out;
    memset(&out, 0, sizeof(out));
    out.src = -1;
    if (best.at >= 0) {
        // (the winner holds min_points >= 3 points: it has a surfel)
        const MmlWmMoments m = wm_moments(W.M.m0[best.at], W.M.m1[best.at], W.M.m2[best.at]);
        float4 o0, o1;
        wm_surfel(m, best.n, o0, o1);
        MmlWmaFactor F;
        if (mml_wma_factor(T, f.x, f.y, f.z, wx, wy, wz, best.cx, best.cy, best.cz, o0.x, o0.y, o0.z, o1.z, O.min_planarity, O.max_dist, F)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                out.ori[c] = F.ori[c];
                out.omega[c] = F.omega[c];
                out.proj[c] = F.proj[c];
            }
            out.error = F.error;
            out.src = i;
        }
    }
    pf[(size_t)slot * MF + i] = out;
}
}  // namespace

void mml_wm_assoc_opts_default(mml_wm_assoc_opts* o, float leaf) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->neighbourhood = 1;
    o->min_points = 5;
    o->min_planarity = 0.5f;
    o->max_plane_dist = (double)leaf;
}
void mml_wm_localize_opts_default(mml_wm_localize_opts* o, float leaf) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    mml_wm_assoc_opts_default(&o->assoc, leaf);
    o->max_plane_dist_by_outer[0] = 2.0 * (double)leaf;
    o->max_plane_dist_by_outer[1] = (double)leaf;
    o->max_plane_dist_by_outer[2] = 0.5 * (double)leaf;
    o->max_outer = 5;
    o->inner_iters = 10;
}

// the refusals of a set of association options, host only
int mml_wm_assoc_opts_ok(mml_ctx* ctx, const char* who, const mml_wm_assoc_opts* o) {
    if (o->neighbourhood != 0 && o->neighbourhood != 1) return mml_refuse(ctx, MML_ERR_INVALID, "%s: neighbourhood %d is neither 0 nor 1", who, o->neighbourhood);
    if (o->min_points < 3) return mml_refuse(ctx, MML_ERR_INVALID, "%s: min_points %d < 3 (a surfel needs three points)", who, o->min_points);
    if (!isfinite(o->min_planarity)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: min_planarity is not finite", who);
    if (!isfinite(o->max_plane_dist) || o->max_plane_dist < 0.0) return mml_refuse(ctx, MML_ERR_INVALID, "%s: max_plane_dist must be finite and >= 0", who);
    return MML_OK;
}

// The refusals of a call that associates slots [first, first + count) against the world map, all before any device work but the
// read-back of the stack sizes, and the call's map numbers sent down (mml_ctx::WorldMap::assoc_maps, one int per slot of the
// context).  need_all: every slot must name a map (mml_world_map_localize).
int mml_wm_assoc_ready(mml_ctx* ctx, const char* who, int first, int count, const int* map_of_slot, const mml_wm_assoc_opts* o, bool need_all) {
    mml_ctx::WorldMap& W = ctx->world;
    if (count < 1 || count > 65535) return mml_refuse(ctx, MML_ERR_INVALID, "%s: count outside 1..65535 (the grid's second dimension)", who);
    if (!map_of_slot || !o) return mml_refuse(ctx, MML_ERR_INVALID, "%s: null map_of_slot / opts", who);
    if (W.n_maps == 0) return mml_refuse(ctx, MML_ERR_STATE, "%s: the context has no world map (mml_world_map_create_opts)", who);
    if (!W.surfels) return mml_refuse(ctx, MML_ERR_STATE, "%s: the world map was created without MML_WM_SURFELS (mml_world_map_create_opts)", who);
    for (int i = 0; i < count; ++i)
        if (map_of_slot[i] < (need_all ? 0 : -1) || map_of_slot[i] >= W.n_maps)
            return mml_refuse(ctx, MML_ERR_INVALID, "%s: map %d of slot %d outside [%d, %d)", who, map_of_slot[i], first + i, need_all ? 0 : -1, W.n_maps);
    int rc = mml_wm_assoc_opts_ok(ctx, who, o);
    if (rc != MML_OK) return rc;
    hipStream_t s = MML_STREAM(ctx);
    int* h = reinterpret_cast<int*>(mml_stage_alloc(ctx, (size_t)ctx->B + 1));  // pinned: the context's 2 B stack sizes
    MML_HIP(hipMemcpyAsync(h, ctx->ft_n, sizeof(int) * 2 * (size_t)ctx->B, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < count; ++i) {
        if (map_of_slot[i] < 0) continue;
        for (int kind = 0; kind < 2; ++kind) {
            const int f = h[(size_t)kind * ctx->B + first + i];
            if (f < 0 || f > ctx->MF) return mml_refuse(ctx, MML_ERR_STATE, "%s: slot %d holds no down-sampled feature stack", who, first + i);
        }
    }
    rc = W.assoc_maps.reserve(ctx, (size_t)ctx->B, s);
    if (rc != MML_OK) return rc;
    int* hm = reinterpret_cast<int*>(mml_stage_alloc(ctx, ((size_t)count + 1) / 2));
    memcpy(hm, map_of_slot, sizeof(int) * (size_t)count);
    MML_HIP(hipMemcpyAsync(W.assoc_maps.d + first, hm, sizeof(int) * (size_t)count, hipMemcpyHostToDevice, s));
    return MML_OK;
}

// the launch: the poses at d_Twl (16 doubles per slot of the call, on the device), the maps as mml_wm_assoc_ready sent them
int mml_launch_wm_associate(mml_ctx* ctx, int first, int count, const double* d_Twl, const mml_wm_assoc_opts& o) {
    mml_ctx::WorldMap& W = ctx->world;
    MmlStageScope t(ctx, "wm_associate");
    const WaTable tab{W.keys, W.slots, W.sum, W.count, WmMom{W.mom[0], W.mom[1], W.mom[2]}};
    const WaOpts opts{mml_wm_inv_leaf(W.leaf), o.neighbourhood, o.min_points, o.min_planarity, o.max_plane_dist};
    hipLaunchKernelGGL(k_wm_associate, dim3((unsigned)((ctx->MF + 255) / 256), (unsigned)count), dim3(256), 0, MML_STREAM(ctx), first, ctx->B, ctx->MF,
                       ctx->ft_n, ctx->ft_xyz[1], W.assoc_maps.d + first, d_Twl, tab, opts, ctx->lf, ctx->pf);
    MML_HIP(hipGetLastError());
    for (int i = 0; i < count; ++i) ctx->stats_stale[first + i] = 1;
    return MML_OK;
}
