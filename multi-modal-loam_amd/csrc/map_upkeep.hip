// Device-side local map upkeep: Estimator::MapIncrementLocal (Estimator.cpp:1585-1643) together with the clear() of
// laserCloud{Corner,Surf}FromLocal that precedes every call (:1083-1085, :1125-1127).
//
// The reference keeps the last localMapWindowSize = 50 key scans' features as 50 PCL clouds in the world frame,
// concatenates them and runs pcl::VoxelGrid over the concatenation; kdtree->setInputCloud then rebuilds both trees on
// the next Estimate() (:1159-1167).  Here the ring lives in HBM next to the scan slots it is fed from, and there is ONE chain,
// written for n maps at once (the end of this file); a single map -- the context's own or one bank of a loop -- is its n = 1 case.
// A segment is (map, kind):
//   k_inc_to_world    : pointAssociateToMap (Map_Manager.cpp:75-89) of a slot's down-sampled stack into ring slot localMapID % 50
//   k_inc_concat_bbox : the ring in slot order = the cloud the filter sees, and its bounding box
//   voxel filter      : PCL voxel index -> ONE stable rocPRIM radix sort of (segment << 32 | index, position) pairs (the points of
//                       a voxel stay in input order = the order the oracle sums them in) -> head flags -> exclusive scan -> one
//                       lane per voxel sums its run and writes the centroid
//   grid build        : the filtered clouds are where mml_build_grids expects them
// Nothing but the cloud sizes and their bounding boxes crosses PCIe.  Compiled with -ffp-contract=off.
#include <math.h>

#include <cstring>
#include <string.h>

#include "mml_internal.h"
#include "voxel_sort_dev.h"

// ---- a10 for labelled clouds beyond the LDS sort of k_voxel: the whole batch through ONE global sort --------------------
// Segment = (slot, kind).  The labelled points of every segment are gathered into one array, keyed by
// (segment << 32 | PCL voxel index in the segment's own grid), sorted by one stable rocPRIM radix sort (a voxel's points
// stay in input order = the order the oracle sums them in), and one lane per voxel writes the centroid to its slot's
// stack.  One 4-byte read-back (the number of labelled points in the batch) is the only host round trip.
namespace {
struct SegParams {
    int first, count, B, NT, MF, list_stride;
    float leaf_corner, leaf_surf;
    const int* fu_info;
    const float4* ln_pts;
    const int* ln_gidx;
    const unsigned* lists;
    const int* glists;  // the listed points' fused indices (label_append)
    int* seg_off;     // 2 * count + 1
    int* seg_bbox;    // 2 * count x 6 order-preserving int keys
    float4* cat;      // gathered points
    unsigned long long* keys;
    unsigned* vals;
    float4* ft0;
    float4* ft1;
    int* ft_n;
};

__global__ void k_seg_prefix(SegParams P, int* total) {
    __shared__ int s_run;
    const int nseg = 2 * P.count;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    // few thousand segments at most: a serial scan by one lane is a few microseconds
    if (threadIdx.x == 0) {
        int run = 0;
        for (int g = 0; g < nseg; ++g) {
            const int b = P.first + (g >> 1), kind = g & 1;
            P.seg_off[g] = run;
            run += P.fu_info[8 * b + 6 + kind];
        }
        P.seg_off[nseg] = run;
        *total = run;
    }
    const int empty[6] = MML_BBOX_EMPTY;
    for (int i = threadIdx.x; i < 6 * nseg; i += blockDim.x) P.seg_bbox[i] = empty[i % 6];
}

// grid (blocks, segment): gather the labelled points and reduce the segment's bounding box
__global__ void k_seg_gather_bbox(SegParams P) {
    const int g = blockIdx.y, b = P.first + (g >> 1), kind = g & 1;
    const int n = P.fu_info[8 * b + 6 + kind], off = P.seg_off[g];
    const unsigned* list = P.lists + ((size_t)b * 2 + kind) * P.list_stride;
    const float4* px = P.ln_pts + (size_t)b * P.NT;
    const int* glist = P.glists + ((size_t)b * 2 + kind) * P.list_stride;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float4 p = px[list[i]];
        p.w = __int_as_float(glist[i]);  // the fused index rides along: it orders the points of a voxel
        P.cat[off + i] = p;
        mn[0] = fminf(mn[0], p.x);
        mn[1] = fminf(mn[1], p.y);
        mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x);
        mx[1] = fmaxf(mx[1], p.y);
        mx[2] = fmaxf(mx[2], p.z);
    }
    if ((int)(blockIdx.x * blockDim.x) >= n) return;  // (the whole workgroup)
    mml_bbox_block_reduce(mn, mx, P.seg_bbox + 6 * g);
}

__global__ void k_seg_keys(SegParams P) {
    const int g = blockIdx.y, kind = g & 1;
    const int off = P.seg_off[g], n = P.seg_off[g + 1] - off;
    const MmlVoxGrid G = mml_vox_grid_of_keys(P.seg_bbox + 6 * g, kind == 0 ? P.leaf_corner : P.leaf_surf);
    const bool unfiltered = n > 0 && G.overflows;  // (PCL returns the cloud as it came)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 p = P.cat[off + i];
        const unsigned idx = G.index(p.x, p.y, p.z);
        // (unfiltered: every point its own voxel, in the order of the fused cloud -- the gathered list is in storage order)
        const unsigned vox = unfiltered ? (unsigned)__float_as_int(p.w) : idx;
        // (segment 12 bits | voxel 32 bits | fused index 20 bits): one sort gives segment, voxel, reference order
        P.keys[off + i] = ((unsigned long long)g << 52) | ((unsigned long long)vox << 20) | (unsigned)__float_as_int(p.w);
        P.vals[off + i] = (unsigned)(off + i);
    }
}

// one lane per voxel; the lane of a segment's first voxel also publishes the segment's voxel count
__global__ void k_seg_centroid(SegParams P, const unsigned long long* keys, const unsigned* vals, const int* flag, const int* pos, int m) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= m || !flag[s]) return;
    const unsigned long long key = keys[s] >> 20;  // (segment, voxel)
    const int g = (int)(key >> 32), b = P.first + (g >> 1), kind = g & 1;
    const int off = P.seg_off[g], end = P.seg_off[g + 1];
    const int dst = pos[s] - pos[off];
    if (s == off) {
        const int nvox = (end < m ? pos[end] : pos[m - 1] + flag[m - 1]) - pos[off];
        P.ft_n[kind * P.B + b] = nvox > P.MF ? -1 : nvox;
    }
    if (dst >= P.MF) return;
    float4 sum;  // (sum.w adds up the fused indices' bit patterns and is not read)
    const float c = static_cast<float>(mml_voxel_run_sum(P.cat, keys, vals, s, m, 20, sum));
    (kind == 0 ? P.ft0 : P.ft1)[(size_t)b * P.MF + dst] = make_float4(sum.x / c, sum.y / c, sum.z / c, 0.f);
}

__global__ void k_seg_empty(SegParams P) {  // segments without labelled points have an empty stack
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 2 * P.count) return;
    if (P.seg_off[g + 1] == P.seg_off[g]) P.ft_n[(g & 1) * P.B + P.first + (g >> 1)] = 0;
}
}  // namespace

int mml_downsample_big(mml_ctx* ctx, int first, int count) {
    // (new stack sizes: statistics computed on demand must not pair the counts written below with an earlier association)
    for (int i = 0; i < count; ++i) ctx->stats_stale[first + i] = 1;
    hipStream_t s = MML_STREAM(ctx);
    const int nseg = 2 * count;
    // scratch for the worst case (every point of every slot labelled), allocated on first use
    const size_t cap = (size_t)ctx->B * ctx->NT;
    if (!ctx->seg_scratch.present()) {
        const int rc = ctx->seg_scratch.reserve(
            ctx, {mml_part(ctx->seg_keys, 2 * cap), mml_part(ctx->seg_vals, 2 * cap), mml_part(ctx->seg_cat, cap), mml_part(ctx->seg_flag, 2 * (cap + 1)),
                  mml_part(ctx->seg_meta, (8 * (size_t)ctx->B * 2 + 16) * mml_ctx::MAX_LANES)});
        if (rc != MML_OK) return mml_refuse(ctx, rc, "mml_downsample_big: out of device memory for the global-sort scratch");
    }
    // lanes work on disjoint slot ranges: each gets the part of the scratch that its slots' points can fill
    const size_t base = (size_t)first * ctx->NT;
    SegParams P;
    P.first = first;
    P.count = count;
    P.B = ctx->B;
    P.NT = ctx->NT;
    P.MF = ctx->MF;
    P.list_stride = ctx->VX_CAP;
    P.leaf_corner = ctx->cfg.leaf_corner;
    P.leaf_surf = ctx->cfg.leaf_surf;
    P.fu_info = ctx->fu_info;
    P.ln_pts = ctx->ln_pts;
    P.ln_gidx = ctx->ln_gidx;
    P.lists = reinterpret_cast<const unsigned*>(ctx->vx_keys);
    P.glists = ctx->vx_gidx;
    int* meta = ctx->seg_meta + (size_t)ctx->cur * (8 * (size_t)ctx->B * 2 + 16);
    P.seg_off = meta + 8;
    P.seg_bbox = meta + 8 + (2 * (size_t)ctx->B + 8);
    int* d_total = meta;
    P.cat = ctx->seg_cat + base;
    P.keys = ctx->seg_keys + base;
    P.vals = ctx->seg_vals + base;
    unsigned long long* keys2 = ctx->seg_keys + cap + base;
    unsigned* vals2 = ctx->seg_vals + cap + base;
    int* flag = ctx->seg_flag + base;
    int* pos = ctx->seg_flag + (cap + 1) + base;
    P.ft0 = ctx->ft_xyz[0];
    P.ft1 = ctx->ft_xyz[1];
    P.ft_n = ctx->ft_n;
    hipLaunchKernelGGL(k_seg_prefix, dim3(1), dim3(256), 0, s, P, d_total);
    int total = 0;
    MML_HIP(hipMemcpyAsync(&total, d_total, sizeof(int), hipMemcpyDeviceToHost, s));
    // (the gather does not depend on the read-back: it runs while the host waits for `total`)
    const int gblocks = (ctx->NT / 4 + 255) / 256 > 0 ? (ctx->NT / 4 + 255) / 256 : 1;
    hipLaunchKernelGGL(k_seg_gather_bbox, dim3(gblocks, nseg), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_seg_keys, dim3(gblocks, nseg), dim3(256), 0, s, P);
    hipLaunchKernelGGL(k_seg_empty, dim3((nseg + 255) / 256), dim3(256), 0, s, P);
    MML_HIP(hipStreamSynchronize(s));
    MML_REQUIRE(total >= 0 && (size_t)total <= (size_t)count * ctx->NT, MML_ERR_STATE, "labelled-point counts of the slots are inconsistent");
    if (total == 0) return MML_OK;
    int seg_bits = 1;
    while ((1 << seg_bits) < nseg) ++seg_bits;
    MML_REQUIRE(ctx->NT <= (1 << 20) && nseg <= 4096, MML_ERR_CAPACITY, "global-sort down-sampler: scans up to 2^20 points, 2048 slots per call");
    int rc = mml_sort_pairs(ctx, ctx->seg_tmp[ctx->cur], P.keys, keys2, P.vals, vals2, (size_t)total, 52 + seg_bits, s);
    if (rc != MML_OK) return rc;
    const int blocks = (total + 255) / 256;
    // (a head = a new (segment, voxel): the key above the fused index's 20 bits)
    hipLaunchKernelGGL(k_run_heads<unsigned long long>, dim3(blocks), dim3(256), 0, s, keys2, total, 20, ~0ull, flag);
    rc = mml_exclusive_scan(ctx, ctx->seg_tmp[ctx->cur], flag, pos, (size_t)total, s);
    if (rc != MML_OK) return rc;
    hipLaunchKernelGGL(k_seg_centroid, dim3(blocks), dim3(256), 0, s, P, keys2, vals2, flag, pos, total);
    MML_HIP(hipGetLastError());
    return MML_OK;
}

// Slots of [first, first + count) that k_voxel marked with ft_n = -1 because a labelled cloud exceeds its LDS sort:
// redone one by one through the global-sort filter.  Synchronises the stream (the marks are read back).  A slot whose
// overflow is a real capacity limit (more voxels than max_features) keeps its mark.
int mml_downsample_redo_overflow(mml_ctx* ctx, int first, int count, std::vector<int>* redone) {
    if (ctx->NT > (1 << 20)) return MML_OK;  // those contexts took the global-sort path to begin with
    hipStream_t s = MML_STREAM(ctx);
    // (pinned destinations: a device-to-host copy into pageable memory is a blocking staged copy, three of them cost more
    //  than the down-sampling kernel of a single scan)
    int* n0 = reinterpret_cast<int*>(mml_stage_alloc(ctx, 5 * (size_t)count + 2));
    int* n1 = n0 + count;
    int* info = n1 + count;
    MML_HIP(hipMemcpyAsync(n0, ctx->ft_n + first, sizeof(int) * count, hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(n1, ctx->ft_n + ctx->B + first, sizeof(int) * count, hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(info, ctx->fu_info + 8 * (size_t)first, sizeof(int) * 8 * (size_t)count, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    for (int c = 0; c < count; ++c) {
        if (n0[c] >= 0 && n1[c] >= 0) continue;
        if (info[8 * c + 6] <= mml_voxel_cap_corner(ctx) && info[8 * c + 7] <= MML_VOXEL_LDS_CAP) continue;  // not a sort overflow
        int rc = mml_downsample_big(ctx, first + c, 1);
        if (rc != MML_OK) return rc;
        if (redone) redone->push_back(first + c);
    }
    return MML_OK;
}

// ---- Estimator::MapIncrementLocal for n maps in one chain of launches ------------------------------------------------------------
// Segment g = 2 i + kind: map i of the chunk, kind.  The chunk's rings are concatenated behind one offset table, the voxel filter
// is mml_downsample_big's pattern (one stable 64-bit radix sort keyed segment << 32 | voxel, one lane per voxel), the grids are
// mml_build_grids'.  A workgroup serves one segment (blockIdx.y): its table row is wave-uniform and comes through scalar loads;
// the sort keeps a segment's points in its own rows [cat_off, cat_off + total), so the kernels behind it index rows the same way.
namespace {
struct IncSegDev {
    double T[12];            // T_wl of the map's slot
    const float4* feat;      // the slot's down-sampled stack of this kind
    float4* ring;            // the map's ring of this kind, LOCAL_WINDOW x MF
    float4* map_out;         // the map's map_tmp + kind * MM
    int n_feat, ring_slot;   // the stack's size, localMapID % 50
    int cat_off, total;      // the segment's rows in the concatenation
    float leaf;
    int ring_off[mml_ctx::LOCAL_WINDOW + 1];  // the ring slots' first rows, relative to cat_off
};

// the slot's stack into ring slot ring_slot, in the world frame
__global__ __launch_bounds__(256) void k_inc_to_world(const IncSegDev* __restrict__ tab, int MF) {
    const IncSegDev& S = tab[blockIdx.y];
    const int n = S.n_feat;
    float4* out = S.ring + (size_t)S.ring_slot * MF;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float4 f = S.feat[i];
        const double x = f.x, y = f.y, z = f.z;
        float4 o;
        o.x = (float)(((S.T[0] * x + S.T[1] * y) + S.T[2] * z) + S.T[3]);
        o.y = (float)(((S.T[4] * x + S.T[5] * y) + S.T[6] * z) + S.T[7]);
        o.z = (float)(((S.T[8] * x + S.T[9] * y) + S.T[10] * z) + S.T[11]);
        o.w = 0.f;
        out[i] = o;
    }
}

// the ring in slot order, one lane per point of the concatenation (the ring slot of a row: upper bound in the segment's 51
// offsets, held in LDS), and the bounding box of what it copies (getMinMax3D of the cloud the filter sees)
__global__ __launch_bounds__(256) void k_inc_concat_bbox(const IncSegDev* __restrict__ tab, int MF, float4* __restrict__ cat,
                                                         int* __restrict__ bbox) {
    constexpr int W = mml_ctx::LOCAL_WINDOW;
    __shared__ int s_off[W + 1];
    const IncSegDev& S = tab[blockIdx.y];
    const int total = S.total;
    if ((int)blockIdx.x * 256 >= total) return;  // (the whole workgroup)
    if (threadIdx.x <= W) s_off[threadIdx.x] = S.ring_off[threadIdx.x];
    __syncthreads();
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        int lo = 0, hi = W;  // the last slot whose offset is <= i (empty slots share an offset: the last of them is the one with points)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= i)
                lo = mid;
            else
                hi = mid;
        }
        const float4 p = S.ring[(size_t)lo * MF + (i - s_off[lo])];
        cat[S.cat_off + i] = p;
        mn[0] = fminf(mn[0], p.x);
        mn[1] = fminf(mn[1], p.y);
        mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x);
        mx[1] = fmaxf(mx[1], p.y);
        mx[2] = fmaxf(mx[2], p.z);
    }
    mml_bbox_block_reduce(mn, mx, bbox + 6 * (size_t)blockIdx.y);
}

// PCL 1.8.1 voxel_grid.hpp applyFilter (MmlVoxGrid): segment << 32 | voxel index in the segment's own box and leaf
__global__ __launch_bounds__(256) void k_inc_voxel_keys(const IncSegDev* __restrict__ tab, const float4* __restrict__ cat,
                                                        const int* __restrict__ bbox, unsigned long long* __restrict__ keys,
                                                        unsigned* __restrict__ vals) {
    const IncSegDev& S = tab[blockIdx.y];
    const int total = S.total, off = S.cat_off;
    if ((int)blockIdx.x * 256 >= total) return;
    const MmlVoxGrid G = mml_vox_grid_of_keys(bbox + 6 * (size_t)blockIdx.y, S.leaf);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const float4 p = cat[off + i];
        const unsigned idx = G.index(p.x, p.y, p.z);
        // (more than INT_MAX voxels in the box: PCL returns the cloud unfiltered = every point its own voxel, in input order)
        keys[off + i] = ((unsigned long long)blockIdx.y << 32) | (G.overflows ? (unsigned)i : idx);
        vals[off + i] = (unsigned)(off + i);
    }
}

// one lane per voxel: AccumulatorXYZ (float sum in input order, then / n) into the map's map_tmp; the lane of the segment's first
// row publishes the segment's voxel count (seg_m was zeroed: a segment without points keeps 0)
__global__ __launch_bounds__(256) void k_inc_centroid(const IncSegDev* __restrict__ tab, const float4* __restrict__ cat,
                                                      const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                                                      const int* __restrict__ flag, const int* __restrict__ pos, int cap,
                                                      int* __restrict__ seg_m) {
    const IncSegDev& S = tab[blockIdx.y];
    const int off = S.cat_off, end = S.cat_off + S.total;
    for (int s = off + blockIdx.x * 256 + threadIdx.x; s < end; s += gridDim.x * 256) {
        if (s == off) seg_m[blockIdx.y] = pos[end - 1] + flag[end - 1] - pos[off];
        if (!flag[s]) continue;
        const int dst = pos[s] - pos[off];
        if (dst >= cap) continue;
        float4 sum;
        const float c = static_cast<float>(mml_voxel_run_sum(cat, keys, vals, s, end, 0, sum));
        S.map_out[dst] = make_float4(sum.x / c, sum.y / c, sum.z / c, 0.f);
    }
}

// the bounding box of every segment's filtered cloud (its size is on the device)
__global__ __launch_bounds__(256) void k_inc_bbox_out(const IncSegDev* __restrict__ tab, const int* __restrict__ seg_m, int cap,
                                                      int* __restrict__ bbox) {
    const float4* pts = tab[blockIdx.y].map_out;
    int m = seg_m[blockIdx.y];
    m = m < cap ? m : cap;
    if ((int)blockIdx.x * 256 >= m) return;  // (the whole workgroup)
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) {
        const float4 p = pts[i];
        mn[0] = fminf(mn[0], p.x);
        mn[1] = fminf(mn[1], p.y);
        mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x);
        mx[1] = fmaxf(mx[1], p.y);
        mx[2] = fmaxf(mx[2], p.z);
    }
    mml_bbox_block_reduce(mn, mx, bbox + 6 * (size_t)blockIdx.y);
}

// what a message calls a map
std::string map_name(const MmlMapState& map) { return map.name < 0 ? std::string("the context's own local map") : "map bank " + std::to_string(map.name); }

// one chunk of maps [i0, i1) of the call: steps 2-4.  nf: the call's 2 n stack sizes.
int increment_chunk(mml_ctx* ctx, int i0, int i1, const MmlMapIncrement* inc, const int* nf, int* n_corner, int* n_surf) {
    constexpr int W = mml_ctx::LOCAL_WINDOW;
    hipStream_t s = MML_STREAM(ctx);
    mml_ctx::BankInc& K = ctx->bank_inc;
    const int nb = i1 - i0, nseg = 2 * nb;
    // the chunk's block, the same layout on the device and in the pinned twin
    MmlCarve<16> carve;
    const MmlField<IncSegDev> f_seg = carve.take<IncSegDev>((size_t)nseg);
    const MmlField<int> f_bbox_in = carve.take<int>(6 * (size_t)nseg);
    const MmlField<int> f_back = carve.take<int>(7 * (size_t)nseg);  // read back in one copy: nseg sizes, nseg filtered boxes
    const size_t up_bytes = carve.bytes();
    const MmlField<char> f_grid = carve.take<char>(mml_grid_table_bytes(nseg));
    IncSegDev* h_seg = f_seg.in(K.tab.h);
    int* h_back = f_back.in(K.tab.h);
    const int empty[6] = MML_BBOX_EMPTY;
    long long total = 0;
    int max_feat = 0, max_total = 0;
    for (int i = i0; i < i1; ++i) {
        MmlMapState& map = *inc[i].map;
        const int Id = (int)(map.local_map_id % W);  // :1597
        for (int kind = 0; kind < 2; ++kind) {
            const int g = 2 * (i - i0) + kind, n = nf[2 * (size_t)i + kind];
            map.ring_n[kind][Id] = n;
            IncSegDev& S = h_seg[g];
            memset(static_cast<void*>(&S), 0, sizeof(S));
            memcpy(S.T, inc[i].T_wl, sizeof(double) * 12);
            S.feat = ctx->ft_xyz[kind] + (size_t)inc[i].slot * ctx->MF;
            S.ring = map.ring[kind];
            S.map_out = map.map_tmp + (size_t)kind * ctx->MM;
            S.n_feat = n;
            S.ring_slot = Id;
            S.leaf = kind == 0 ? ctx->cfg.leaf_corner : ctx->cfg.leaf_surf;
            for (int r = 0; r < W; ++r) S.ring_off[r + 1] = S.ring_off[r] + map.ring_n[kind][r];
            S.cat_off = (int)total;
            S.total = S.ring_off[W];
            total += S.total;
            if (n > max_feat) max_feat = n;
            if (S.total > max_total) max_total = S.total;
            for (int c = 0; c < 6; ++c) f_bbox_in.in(K.tab.h)[6 * (size_t)g + c] = h_back[nseg + 6 * (size_t)g + c] = empty[c];
            h_back[g] = 0;
        }
    }
    MML_REQUIRE(total <= (long long)K.cap, MML_ERR_CAPACITY, "local-map increment: more ring points than the scratch holds");
    MML_HIP(hipMemcpyAsync(K.tab.d, K.tab.h, up_bytes, hipMemcpyHostToDevice, s));
    const IncSegDev* d_seg = f_seg.in(K.tab.d);
    int* d_bbox_in = f_bbox_in.in(K.tab.d);
    int* d_seg_m = f_back.in(K.tab.d);
    int* d_bbox_out = d_seg_m + nseg;
    unsigned long long* keys2 = K.keys + K.cap;
    unsigned* vals2 = K.vals + K.cap;
    int* flag = K.flag;
    int* pos = K.flag + K.cap + 1;
    auto blocks_for = [](int n) { return n > 0 ? ((n + 255) / 256 < 256 ? (n + 255) / 256 : 256) : 1; };
    if (max_feat) hipLaunchKernelGGL(k_inc_to_world, dim3(blocks_for(max_feat), nseg), dim3(256), 0, s, d_seg, ctx->MF);
    if (total) {
        const int blocks = blocks_for(max_total);
        hipLaunchKernelGGL(k_inc_concat_bbox, dim3(blocks, nseg), dim3(256), 0, s, d_seg, ctx->MF, K.cat, d_bbox_in);
        hipLaunchKernelGGL(k_inc_voxel_keys, dim3(blocks, nseg), dim3(256), 0, s, d_seg, K.cat, d_bbox_in, K.keys, K.vals);
        int seg_bits = 1;
        while ((1 << seg_bits) < nseg) ++seg_bits;
        int rc = mml_sort_pairs(ctx, ctx->sort_tmp, K.keys, keys2, K.vals, vals2, (size_t)total, 32 + seg_bits, s);
        if (rc != MML_OK) return rc;
        hipLaunchKernelGGL(k_run_heads<unsigned long long>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, keys2, (int)total, 0,
                           ~0ull, flag);
        rc = mml_exclusive_scan(ctx, ctx->sort_tmp, flag, pos, (size_t)total, s);
        if (rc != MML_OK) return rc;
        hipLaunchKernelGGL(k_inc_centroid, dim3(blocks, nseg), dim3(256), 0, s, d_seg, K.cat, keys2, vals2, flag, pos, ctx->MM, d_seg_m);
        hipLaunchKernelGGL(k_inc_bbox_out, dim3(blocks, nseg), dim3(256), 0, s, d_seg, d_seg_m, ctx->MM, d_bbox_out);
    }
    MML_HIP(hipMemcpyAsync(h_back, d_seg_m, f_back.bytes(), hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));  // the chunk's second synchronisation of 2 + R (the first read the stack sizes)
    for (int g = 0; g < nseg; ++g)
        if (h_back[g] > ctx->MM)
            return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: filtered local map larger than max_map_points", map_name(*inc[i0 + g / 2].map).c_str());
    std::vector<MmlGridJob> jobs((size_t)nseg);
    for (int g = 0; g < nseg; ++g) {
        MmlMapState& map = *inc[i0 + g / 2].map;
        const int kind = g & 1;
        map.have_map[kind] = false;  // (mml_build_grid)
        map.grid[kind].tags = nullptr;
        jobs[g] = MmlGridJob{&map.grid[kind], map.map_tmp + (size_t)kind * ctx->MM, kind == 0 ? ctx->cfg.cell_corner : ctx->cfg.cell_surf,
                             h_back[g], h_back + nseg + 6 * (size_t)g, nullptr};
    }
    ctx->banks.dirty = true;  // (the descriptor table of a context with banks holds a copy of these grids)
    const MmlGridScratch<unsigned long long> G{K.keys, keys2, K.vals, vals2, K.cap, f_grid.in(K.tab.d), f_grid.in(K.tab.h)};
    int rounds = 0;
    const int rc = mml_build_grids(ctx, nseg, jobs.data(), G, &rounds);
    if (rc != MML_OK) return rc;
    for (int i = i0; i < i1; ++i) {
        MmlMapState& map = *inc[i].map;
        for (int kind = 0; kind < 2; ++kind) {
            map.have_map[kind] = true;
            map.local_map_n[kind] = h_back[2 * (i - i0) + kind];
        }
        if (n_corner) n_corner[i] = map.local_map_n[0];
        if (n_surf) n_surf[i] = map.local_map_n[1];
        ++map.local_map_id;  // :1642
    }
    return MML_OK;
}
}  // namespace

int mml_map_upkeep_increment_segmented(mml_ctx* ctx, int n, const MmlMapIncrement* inc, int* n_corner, int* n_surf) {
    constexpr int W = mml_ctx::LOCAL_WINDOW;
    hipStream_t s = MML_STREAM(ctx);
    mml_ctx::BankInc& K = ctx->bank_inc;
    // step 1: the stack sizes in one copy (the context's 2 B ints), those of the n slots checked before a map changes
    std::vector<int> nf(2 * (size_t)n);
    {
        int* h = reinterpret_cast<int*>(mml_stage_alloc(ctx, (size_t)ctx->B + 1));  // pinned
        MML_HIP(hipMemcpyAsync(h, ctx->ft_n, sizeof(int) * 2 * (size_t)ctx->B, hipMemcpyDeviceToHost, s));
        MML_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i)
            for (int kind = 0; kind < 2; ++kind) nf[2 * (size_t)i + kind] = h[(size_t)kind * ctx->B + inc[i].slot];
    }
    for (int i = 0; i < n; ++i)
        for (int kind = 0; kind < 2; ++kind) {
            const int f = nf[2 * (size_t)i + kind];
            if (f < 0 || f > ctx->MF) return mml_refuse(ctx, MML_ERR_STATE, "slot %d holds no down-sampled feature stack", inc[i].slot);
        }
    // every segment's ring total after the write, the filter's own limit and the chunks: greedy, in call order
    std::vector<long long> pts((size_t)n);
    for (int i = 0; i < n; ++i) {
        MmlMapState& map = *inc[i].map;
        const int Id = (int)(map.local_map_id % W);
        pts[i] = 0;
        for (int kind = 0; kind < 2; ++kind) {
            long long t = nf[2 * (size_t)i + kind];
            for (int r = 0; r < W; ++r)
                if (r != Id) t += map.ring_n[kind][r];
            if (t > ctx->MM) return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: cloud larger than max_map_points", map_name(map).c_str());
            pts[i] += t;
        }
    }
    std::vector<int> cut(1, 0);  // chunk c = maps [cut[c], cut[c + 1]) of the call
    long long run = 0, max_pts = 1;
    int max_maps = 1;
    for (int i = 0; i < n; ++i) {
        if (i > cut.back() && run + pts[i] > K.budget) {
            cut.push_back(i);
            run = 0;
        }
        run += pts[i];
        if (run > max_pts) max_pts = run;
        if (i + 1 - cut.back() > max_maps) max_maps = i + 1 - cut.back();
    }
    cut.push_back(n);
    MML_REQUIRE(max_pts < (1ll << 31), MML_ERR_CAPACITY, "local-map increment: a chunk's rings exceed 2^31 points");
    // memory: the maps' rings (a first increment), the scratch for the largest chunk, its tables, the sort's temporary storage --
    // all before the first launch, so that nothing is replaced while a chunk's kernels run
    const size_t ring_pts = (size_t)W * ctx->MF;
    for (int i = 0; i < n; ++i) {
        MmlMapState& map = *inc[i].map;
        if (map.ring_mem.present()) continue;
        const int rc = map.ring_mem.reserve(ctx, {mml_part(map.ring[0], ring_pts), mml_part(map.ring[1], ring_pts)});
        if (rc != MML_OK) return rc;
    }
    if ((size_t)max_pts > K.cap || !K.mem.present()) {
        const size_t cap = (size_t)max_pts;
        K.cap = 0;
        const int rc = K.mem.reserve(ctx, {mml_part(K.cat, cap), mml_part(K.keys, 2 * cap), mml_part(K.vals, 2 * cap), mml_part(K.flag, 2 * (cap + 1))});
        if (rc != MML_OK) return rc;
        K.cap = cap;
    }
    {
        const size_t nseg = 2 * (size_t)max_maps;
        const size_t bytes = sizeof(IncSegDev) * nseg + sizeof(int) * 13 * nseg + mml_grid_table_bytes((int)nseg) + 16 * 8;
        int rc = K.tab.reserve(ctx, bytes);
        if (rc != MML_OK) return rc;
        int seg_bits = 1;
        while ((1u << seg_bits) < nseg) ++seg_bits;
        rc = ctx->sort_tmp.reserve(ctx, mml_sort_pairs_bytes<unsigned long long>((size_t)max_pts, 32 + seg_bits, s));
        if (rc != MML_OK) return rc;
    }
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const int rc = increment_chunk(ctx, cut[c], cut[c + 1], inc, nf.data(), n_corner, n_surf);
        if (rc != MML_OK) return rc;
    }
    MML_HIP(hipGetLastError());
    return MML_OK;
}
