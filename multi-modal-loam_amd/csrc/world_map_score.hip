// world_map_score.hip -- pose hypotheses scored against a surfel world map (mml_world_map_score, and the levels of
// mml_world_map_relocalize): H hypotheses for each of `count` slots in ONE launch.  The arithmetic of a feature is
// world_map_score.h's (which is world_map_assoc.h's up to the gates) and nowhere else; the candidate walk is wm_probe27, the one
// k_wm_associate runs; the winner's normal and planarity come from the map's surfel cache (world_map.hip mml_wm_cache_ready).
//
// k_wm_score  grid (ceil(H / 4), count), 256 lanes: ONE wavefront per (slot, hypothesis).  The wave's number inside the workgroup
//             is made uniform with readfirstlane, so the slot's map, its stack size and the 12 pose entries of the hypothesis are
//             indexed by scalars alone (blockIdx, the wave number) through const __restrict__ parameters, before the first store.
//             The wave walks the slot's features 64 at a time (feature t * stride in lane t mod 64); a lane keeps two 64-bit
//             integer accumulators (score_q; n_match and n_scored packed into one word).  One butterfly over the wave's lanes
//             (cross-lane moves, no LDS allocated), one 16-byte store by lane 0.  No atomics, no zeroing pass: every (slot,
//             hypothesis) of the grid stores its result, zeros for a skipped slot.
// Host: the hypotheses go down from the pinned twin of the call's block (MML_SIDE_WM_SCORE), the results come up into it: ONE host
// synchronisation behind the launch, beside the read-back of the stack sizes at entry (mml_wm_assoc_ready).
#include <math.h>
#include <string.h>

#include "mml_internal.h"
#include "world_map_score.h"

static_assert(sizeof(mml_wm_score) == 16, "one 16-byte store per result");

struct MmlWmScoreDev {
    MmlStaging<char> io;  // down: count x n_hyp x 16 doubles; up: count x n_hyp results
    ~MmlWmScoreDev() { io.release(); }
};

namespace {
#include "eig3_dev.h"
#include "world_map_dev.h"

struct WsTable {
    const unsigned long long* keys;
    unsigned long long slots;
    const float4* sum;
    const int* count;
    const float4* cache;
};
struct WsOpts {
    float inv;
    int nb, min_points;
    float min_planarity;
    double max_dist;
    int stride;
};

__global__ __launch_bounds__(256) void k_wm_score(int first, int B, int MF, int H, const int* __restrict__ ft_n, const float4* __restrict__ ft,
                                                  const int* __restrict__ maps, const double* __restrict__ Twl, WsTable W, WsOpts O,
                                                  ulonglong2* __restrict__ out) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int hyp = (int)blockIdx.x * 4 + wave;
    if (hyp >= H) return;  // (the whole wave)
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.y * (size_t)H + (size_t)hyp;
    const int map = maps[blockIdx.y];
    const int slot = first + blockIdx.y;
    int ns = ft_n[B + slot];
    ns = ns < 0 ? 0 : (ns > MF ? MF : ns);  // (the host refused a slot without a stack; an index stays inside the slot's MF)
    double T[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) T[c] = Twl[16 * row + c];
    MmlWmsAcc acc;
    mml_wms_init(acc);
    const int n = map < 0 ? 0 : mml_wms_count(ns, O.stride);
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane;
        if (t >= n) continue;
        const float4 f = ft[(size_t)slot * MF + mml_wms_feature(t, O.stride)];
        float wx, wy, wz;
        mml_world_point(T, f.x, f.y, f.z, wx, wy, wz);
        int vi = 0, vj = 0, vk = 0;
        if (!mml_wma_voxel(wx, wy, wz, O.inv, vi, vj, vk)) continue;
        MmlWmaBest best;
        mml_wma_best_init(best);
        wm_probe27(W.keys, W.slots, W.sum, W.count, map, O.nb, O.min_points, vi, vj, vk, wx, wy, wz, best);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (best.at >= 0) s = W.cache[best.at];
        mml_wms_add(acc, wx, wy, wz, best, s.x, s.y, s.z, s.w, O.min_planarity, O.max_dist);
    }
    unsigned long long q = acc.score_q, c = (unsigned long long)(unsigned)acc.n_match | ((unsigned long long)(unsigned)acc.n_scored << 32);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        q += __shfl_xor(q, m, 64);
        c += __shfl_xor(c, m, 64);
    }
    if (lane == 0) out[row] = make_ulonglong2(q, c);  // {score_q, n_match | n_scored << 32}: mml_wm_score's 16 bytes
}
}  // namespace

void mml_wm_score_opts_default(mml_wm_score_opts* o, float leaf) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    mml_wm_assoc_opts_default(&o->assoc, leaf);
    o->stride = 1;
}

int mml_wm_score_run(mml_ctx* ctx, const char* who, int first, int count, const int* map_of_slot, int n_hyp, const double* T_wl,
                     const mml_wm_score_opts* o, mml_wm_score* out, bool ready) {
    mml_ctx::WorldMap& W = ctx->world;
    if (!T_wl || !out || !o) return mml_refuse(ctx, MML_ERR_INVALID, "%s: null T_wl / out / opts", who);
    if (n_hyp < 1 || n_hyp > 65536) return mml_refuse(ctx, MML_ERR_INVALID, "%s: n_hyp %d outside 1..65536", who, n_hyp);
    if (count >= 1 && (long long)count * n_hyp > (1LL << 22))
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: count %d x n_hyp %d exceeds 2^22 hypotheses per call", who, count, n_hyp);
    if (o->stride < 1) return mml_refuse(ctx, MML_ERR_INVALID, "%s: stride %d < 1", who, o->stride);
    if (!(isfinite(o->assoc.max_plane_dist) && o->assoc.max_plane_dist > 0.0))
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: max_plane_dist must be finite and > 0 (the score divides by it)", who);
    int rc = ready ? mml_wm_assoc_ready(ctx, who, first, count, map_of_slot, &o->assoc, false) : MML_OK;
    if (rc != MML_OK) return rc;
    hipStream_t s = MML_STREAM(ctx);
    const size_t rows = (size_t)count * (size_t)n_hyp;
    MmlCarve<16> c;
    const MmlField<double> f_T = c.take<double>(16 * rows);
    const MmlField<mml_wm_score> f_out = c.take<mml_wm_score>(rows);
    MmlWmScoreDev* d = mml_side<MmlWmScoreDev>(ctx, MML_SIDE_WM_SCORE);
    rc = d->io.reserve(ctx, c.bytes(), s);
    if (rc != MML_OK) return rc;
    rc = mml_wm_cache_ready(ctx);  // (allocates before any launch; the rebuild of a stale cache is enqueued in front of the score)
    if (rc != MML_OK) return rc;
    // (the pinned twin is free: the last call that used it waited for its read-back)
    memcpy(f_T.in(d->io.h), T_wl, f_T.bytes());
    MML_HIP(hipMemcpyAsync(f_T.in(d->io.d), f_T.in(d->io.h), f_T.bytes(), hipMemcpyHostToDevice, s));
    {
        MmlStageScope t(ctx, "wm_score");
        const WsTable tab{W.keys, W.slots, W.sum, W.count, W.cache};
        const WsOpts opts{mml_wm_inv_leaf(W.leaf), o->assoc.neighbourhood, o->assoc.min_points, o->assoc.min_planarity, o->assoc.max_plane_dist, o->stride};
        hipLaunchKernelGGL(k_wm_score, dim3((unsigned)((n_hyp + 3) / 4), (unsigned)count), dim3(256), 0, s, first, ctx->B, ctx->MF, n_hyp, ctx->ft_n,
                           ctx->ft_xyz[1], W.assoc_maps.d + first, f_T.in(d->io.d), tab, opts, reinterpret_cast<ulonglong2*>(f_out.in(d->io.d)));
        MML_HIP(hipGetLastError());
    }
    MML_HIP(hipMemcpyAsync(f_out.in(d->io.h), f_out.in(d->io.d), f_out.bytes(), hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));  // the call's one synchronisation behind the launch
    memcpy(out, f_out.in(d->io.h), f_out.bytes());
    return MML_OK;
}
