// map_global.hip -- SURVEY.md section 8(f) rank 2, global half: the MAP_MANAGER corner / surf cube stores on the device, the
// context's own store and every map bank's (include/mmloam_hip.h) through ONE chain of launches for n stores:
//   MAP_MANAGER::featureAssociateToMap (Map_Manager.cpp:91-117)  -> mml_cube_store_append_segmented      (features of n slots -> world)
//   MAP_MANAGER::MapIncrement (:125-281) + MapMove (:288-581)     -> mml_cube_store_increment_segmented
// The own-map calls (map_banks.hip) are the chain with n = 1 on mml_ctx::own; there is no other implementation.
// The reference keeps 4851 PCL clouds per kind and rotates pointers between them; here a store is ONE array of points with a
// 16-bit cube tag each (the layout k_associate consumes, a12):
//   * MapMove becomes per-axis counts of layer shifts applied to the tags; a point whose layer leaves the 21 x 21 x 11 grid is
//     dropped (the reference clears the cube that wraps around);
//   * new points are tagged with the shifted centre, per-cube counts come from a histogram, cubes that received points and now hold
//     > 300 are voxel-filtered (:225-233) -- all of them in one pass: per-cube bounding boxes through atomics, 64-bit keys, one
//     stable radix sort, one lane per voxel;
//   * points of untouched cubes keep their relative order, filtered cubes are re-emitted in voxel order, new points of small cubes
//     follow the old ones: the order inside every cube equals the reference's, which is what fixes the tie order of the exact 5-NN.
// What Estimate() matches against is the state at the START of the last MapIncrement (laserCloud*_for_match, laserCloudCen*_last,
// :136-149): the match copy is built from the store BEFORE it is updated.
// A SEGMENT is (store of the call, kind): 2 n of them.  Their points lie behind one offset table in one combined index space --
// segment g's rows are [off, off + n0 + np), the store first, then the pending points -- and a workgroup serves one segment
// (blockIdx.y), so its table row is wave-uniform.  Per chunk of stores (the chunk rule: mml_cube_chunks below):
//   tag + histogram   the cube of every row -- a stored point's tag with the MapMove shifts applied AS IT IS READ, a pending point's
//                     from the moved centre -- into scratch, and the per-(segment, cube) counts and `changed` flags;
//   classify          keep (valid, cube not filtered) / selected (cube changed and > 300 points, Map_Manager.cpp:225);
//   2 scans           ONE exclusive scan per flag array over all segments; a segment's bases are the scan values at its start;
//   read-back 1       every segment's keep / selected totals: the CAPACITY DECISION, taken before anything but scratch is written;
//   scatter           kept rows into the store's second buffer (shifted tags), selected rows into scratch, per-(segment, cube) boxes;
//   keys, sort        segment << 53 | cube << 40 | PCL voxel index, ONE stable sort over 53 + bits(segments) bits;
//   heads, scan, centroids, read-back 2: the filtered sizes.
// The live arrays, their tags, the centres and the pending counts are READ ONLY until every chunk has passed its capacity decision
// and its chain; the match copies (the stores as they were at the start, with the centres before MapMove) are then built from the
// untouched arrays by mml_build_grids -- one bounding-box read-back, one per refinement round -- and only then are the buffers
// swapped and the host state written.  Every refusal therefore leaves all n stores exactly as they were.
// Compiled with -ffp-contract=off.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mml_internal.h"
#include "voxel_sort_dev.h"

namespace {

constexpr int NCUBE = 4851;
constexpr uint16_t DEAD = 0xFFFFu;
constexpr int SEG_INTS = 8 * NCUBE;  // per segment: cnt | changed | six box keys per cube

// One row per segment.  MapMove's shift list is, per axis, `up` shifts by +1 followed by `down` shifts by -1 (the two while loops
// of Map_Manager.cpp:288-581 in their order); a layer that leaves the grid on the way is dropped: after the ups the layer must be
// below the limit, after the downs at or above 0 -- the same points die as when the list is walked shift by shift.
struct CubeSegDev {
    const float4* spts;    // the live store: read only
    const uint16_t* stag;
    float4* out_pts;       // its second buffer
    uint16_t* out_tag;
    const float4* ppts;    // the pending points
    float4* m_pts;         // the match copy's unsorted cloud, tags and cube counts (the match phase)
    uint16_t* m_tag;
    int* m_cnt;
    int n0, np, off;
    int cen[3];            // the centre AFTER MapMove: Width, Height, Depth
    int up[3], down[3];    // per axis I, J, K
    int _pad;
};
static_assert(sizeof(CubeSegDev) % 8 == 0, "rows are packed behind one another");

struct CubeAppDev {  // the append: one row per (slot, kind)
    const float4* feat;
    float4* out;
    double T[12];
    int n, _pad;
};

__device__ __forceinline__ int shifted_tag(int t, const CubeSegDev& S) {
    if (t == DEAD) return DEAD;
    int c[3] = {t % 21, (t / 21) % 21, t / 441};
    const int lim[3] = {21, 21, 11};
    bool dead = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int hi = c[a] + S.up[a];
        c[a] = hi - S.down[a];
        dead = dead || hi >= lim[a] || c[a] < 0;
    }
    return dead ? (int)DEAD : c[0] + 21 * c[1] + 441 * c[2];
}

// cube of a new world-frame point (Map_Manager.cpp:159-176), DEAD outside the grid
__device__ __forceinline__ int tag_of_point(const float4 p, int cenW, int cenH, int cenD) {
    int cubeI = int((p.x + 25.0) / 50.0) + cenD;
    int cubeJ = int((p.y + 25.0) / 50.0) + cenW;
    int cubeK = int((p.z + 25.0) / 50.0) + cenH;
    if (p.x + 25.0 < 0) cubeI--;
    if (p.y + 25.0 < 0) cubeJ--;
    if (p.z + 25.0 < 0) cubeK--;
    const bool ok = cubeI >= 0 && cubeI < 21 && cubeJ >= 0 && cubeJ < 21 && cubeK >= 0 && cubeK < 11;
    return ok ? cubeI + 21 * cubeJ + 441 * cubeK : (int)DEAD;
}

__global__ __launch_bounds__(256) void k_cs_to_world(const CubeAppDev* __restrict__ tab) {
    const CubeAppDev& S = tab[blockIdx.y];
    const int n = S.n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float4 f = S.feat[i];
        const double x = f.x, y = f.y, z = f.z;
        float4 o;
        o.x = (float)(((S.T[0] * x + S.T[1] * y) + S.T[2] * z) + S.T[3]);
        o.y = (float)(((S.T[4] * x + S.T[5] * y) + S.T[6] * z) + S.T[7]);
        o.z = (float)(((S.T[8] * x + S.T[9] * y) + S.T[10] * z) + S.T[11]);
        o.w = 0.f;
        S.out[i] = o;
    }
}

// the cube of every row of the combined index space, and the segment's histogram (cnt, changed: zeroed by the host)
__global__ __launch_bounds__(256) void k_cs_tag_hist(const CubeSegDev* __restrict__ tab, uint16_t* __restrict__ tag, int* __restrict__ cnt,
                                                     int* __restrict__ changed) {
    const CubeSegDev& S = tab[blockIdx.y];
    const int n0 = S.n0, nu = S.n0 + S.np, off = S.off;
    int* c = cnt + (size_t)blockIdx.y * NCUBE;
    int* ch = changed + (size_t)blockIdx.y * NCUBE;
    for (int u = blockIdx.x * 256 + threadIdx.x; u < nu; u += gridDim.x * 256) {
        const int t = u < n0 ? shifted_tag(S.stag[u], S) : tag_of_point(S.ppts[u - n0], S.cen[0], S.cen[1], S.cen[2]);
        tag[off + u] = (uint16_t)t;
        if (t == DEAD) continue;
        atomicAdd(&c[t], 1);
        if (u >= n0) ch[t] = 1;
    }
}

__global__ __launch_bounds__(256) void k_cs_classify(const CubeSegDev* __restrict__ tab, const uint16_t* __restrict__ tag,
                                                     const int* __restrict__ cnt, const int* __restrict__ changed, int* __restrict__ keep,
                                                     int* __restrict__ sel) {
    const CubeSegDev& S = tab[blockIdx.y];
    const int nu = S.n0 + S.np, off = S.off;
    const int* c = cnt + (size_t)blockIdx.y * NCUBE;
    const int* ch = changed + (size_t)blockIdx.y * NCUBE;
    for (int u = blockIdx.x * 256 + threadIdx.x; u < nu; u += gridDim.x * 256) {
        const int t = tag[off + u];
        const bool valid = t != DEAD;
        const bool filt = valid && ch[t] && c[t] > 300;  // :225
        keep[off + u] = (valid && !filt) ? 1 : 0;
        sel[off + u] = filt ? 1 : 0;
    }
}

// per segment: kept rows | selected rows | first selected row in the selected concatenation   (back: 4 x nseg ints, the last nseg
// the filtered sizes k_cs_centroid writes)
__global__ void k_cs_totals(const CubeSegDev* __restrict__ tab, int nseg, const int* __restrict__ keep, const int* __restrict__ keep_pos,
                            const int* __restrict__ sel, const int* __restrict__ sel_pos, int* __restrict__ back) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nseg) return;
    const int off = tab[g].off, end = off + tab[g].n0 + tab[g].np;
    const bool any = end > off;
    back[g] = any ? keep_pos[end - 1] + keep[end - 1] - keep_pos[off] : 0;
    back[nseg + g] = any ? sel_pos[end - 1] + sel[end - 1] - sel_pos[off] : 0;
    back[2 * nseg + g] = any ? sel_pos[off] : 0;
}

__global__ void k_cs_init_bbox(int* bbox, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int empty[6] = MML_BBOX_EMPTY;
    bbox[i] = empty[i % 6];
}

__global__ __launch_bounds__(256) void k_cs_scatter(const CubeSegDev* __restrict__ tab, const uint16_t* __restrict__ tag,
                                                    const int* __restrict__ keep, const int* __restrict__ keep_pos,
                                                    const int* __restrict__ sel, const int* __restrict__ sel_pos, float4* __restrict__ sel_pts,
                                                    uint16_t* __restrict__ sel_tag, int* __restrict__ bbox /* nseg x NCUBE x 6 keys */) {
    const CubeSegDev& S = tab[blockIdx.y];
    const int n0 = S.n0, nu = S.n0 + S.np, off = S.off;
    if ((int)blockIdx.x * 256 >= nu) return;  // (the whole workgroup; keep_pos[off] below is a row of this segment)
    const int kb = keep_pos[off];
    int* box = bbox + (size_t)blockIdx.y * (6 * NCUBE);
    for (int u = blockIdx.x * 256 + threadIdx.x; u < nu; u += gridDim.x * 256) {
        const float4 p = u < n0 ? S.spts[u] : S.ppts[u - n0];
        const uint16_t t = tag[off + u];
        if (keep[off + u]) {
            const int d = keep_pos[off + u] - kb;
            S.out_pts[d] = p;
            S.out_tag[d] = t;
        } else if (sel[off + u]) {
            const int d = sel_pos[off + u];
            sel_pts[d] = p;
            sel_tag[d] = t;
            int* b = box + 6 * (int)t;  // getMinMax3D of the cube's cloud
            atomicMin(b + 0, mml_fkey(p.x));
            atomicMin(b + 1, mml_fkey(p.y));
            atomicMin(b + 2, mml_fkey(p.z));
            atomicMax(b + 3, mml_fkey(p.x));
            atomicMax(b + 4, mml_fkey(p.y));
            atomicMax(b + 5, mml_fkey(p.z));
        }
    }
}

// PCL 1.8.1 voxel_grid.hpp applyFilter, per (segment, cube): the key of mml_cube_key below
__global__ __launch_bounds__(256) void k_cs_vox_keys(const int* __restrict__ back, int nseg, const float4* __restrict__ sel_pts,
                                                     const uint16_t* __restrict__ sel_tag, const int* __restrict__ bbox, float leaf,
                                                     unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
    const int ns = back[nseg + blockIdx.y], sb = back[2 * nseg + blockIdx.y];
    const int* box = bbox + (size_t)blockIdx.y * (6 * NCUBE);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < ns; i += gridDim.x * 256) {
        const int j = sb + i;
        const int t = sel_tag[j];
        const MmlVoxGrid g = mml_vox_grid_of_keys(box + 6 * t, leaf);  // (no overflow fall-back, as in the one-store chain)
        const float4 p = sel_pts[j];
        keys[j] = mml_cube_key(blockIdx.y, (unsigned)t, g.index(p.x, p.y, p.z));
        vals[j] = (unsigned)j;
    }
}

// one lane per voxel into the second buffer behind the segment's kept rows; the lane of the segment's first row publishes its
// filtered size (zeroed by the host: a segment without selected rows keeps 0)
__global__ __launch_bounds__(256) void k_cs_centroid(const CubeSegDev* __restrict__ tab, int* __restrict__ back, int nseg,
                                                     const float4* __restrict__ sel_pts, const unsigned long long* __restrict__ keys,
                                                     const unsigned* __restrict__ vals, const int* __restrict__ flag, const int* __restrict__ pos,
                                                     int cap) {
    const CubeSegDev& S = tab[blockIdx.y];
    const int nk = back[blockIdx.y], ns = back[nseg + blockIdx.y], sb = back[2 * nseg + blockIdx.y];
    if ((int)blockIdx.x * 256 >= ns) return;  // (the whole workgroup; pos[sb] below is a row of this segment)
    const int end = sb + ns, pb = pos[sb];
    for (int s = sb + blockIdx.x * 256 + threadIdx.x; s < end; s += gridDim.x * 256) {
        if (s == sb) back[3 * nseg + blockIdx.y] = pos[end - 1] + flag[end - 1] - pb;
        if (!flag[s]) continue;
        const int dst = nk + (pos[s] - pb);
        if (dst >= cap) continue;
        const unsigned long long key = keys[s];
        float4 sum;
        const float c = static_cast<float>(mml_voxel_run_sum(sel_pts, keys, vals, s, end, 0, sum));
        S.out_pts[dst] = make_float4(sum.x / c, sum.y / c, sum.z / c, 0.f);
        S.out_tag[dst] = (uint16_t)mml_cube_key_cube(key);
    }
}

__global__ __launch_bounds__(256) void k_cs_zero_cnt(const CubeSegDev* __restrict__ tab) {
    int* c = tab[blockIdx.y].m_cnt;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < NCUBE; i += gridDim.x * 256) c[i] = 0;
}

// the match copy's unsorted cloud, tags and cube counts from the live store as it is, and the cloud's bounding box
__global__ __launch_bounds__(256) void k_cs_match_copy(const CubeSegDev* __restrict__ tab, int* __restrict__ bbox) {
    const CubeSegDev& S = tab[blockIdx.y];
    const int n0 = S.n0;
    if ((int)blockIdx.x * 256 >= n0) return;  // (the whole workgroup)
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n0; i += gridDim.x * 256) {
        const float4 p = S.spts[i];
        const uint16_t t = S.stag[i];
        S.m_pts[i] = p;
        S.m_tag[i] = t;
        if (t != DEAD) atomicAdd(S.m_cnt + t, 1);
        mn[0] = fminf(mn[0], p.x);
        mn[1] = fminf(mn[1], p.y);
        mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x);
        mx[1] = fmaxf(mx[1], p.y);
        mx[2] = fmaxf(mx[2], p.z);
    }
    mml_bbox_block_reduce(mn, mx, bbox + 6 * (size_t)blockIdx.y);
}

int blocks_for(int n) { return n > 0 ? ((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024) : 1; }

// MapMove (Map_Manager.cpp:288-581) on a host copy of the centre: the layer shifts that keep the sensor's cube 8 cubes away from
// every face (at most 64), counted per axis and direction.  The one MapMove planner.
struct Move {
    int cen[3];
    int up[3], down[3];
};
int plan_move(mml_ctx* ctx, const int* cen_now, const double* T_wl, Move& M) {
    int cen[3] = {cen_now[0], cen_now[1], cen_now[2]};
    int n_shift = 0;
    const double t[3] = {T_wl[3], T_wl[7], T_wl[11]};
    int c[3] = {int((t[0] + 25.0) / 50.0) + cen[2], int((t[1] + 25.0) / 50.0) + cen[0], int((t[2] + 25.0) / 50.0) + cen[1]};
    for (int a = 0; a < 3; ++a)
        if (t[a] + 25.0 < 0) c[a]--;
    const int lim[3] = {21, 21, 11};
    int* cen_of_axis[3] = {&cen[2], &cen[0], &cen[1]};  // I <-> Depth, J <-> Width, K <-> Height
    for (int a = 0; a < 3; ++a) {
        M.up[a] = M.down[a] = 0;
        while (c[a] < 8) {
            MML_REQUIRE(n_shift < 64, MML_ERR_INVALID, "pose far outside the cube grid");
            ++n_shift, ++M.up[a], ++c[a], ++*cen_of_axis[a];
        }
        while (c[a] >= lim[a] - 8) {
            MML_REQUIRE(n_shift < 64, MML_ERR_INVALID, "pose far outside the cube grid");
            ++n_shift, ++M.down[a], --c[a], --*cen_of_axis[a];
        }
    }
    for (int k = 0; k < 3; ++k) M.cen[k] = cen[k];
    return MML_OK;
}

// a refusal that names the map's store: a bank, or the text alone for the context's own
int refuse_store(mml_ctx* ctx, int code, const MmlMapState& map, const char* what) {
    return map.name < 0 ? mml_refuse(ctx, code, "%s", what) : mml_refuse(ctx, code, "map bank %d: %s", map.name, what);
}

// what the chain of one chunk leaves on the host for the commit
struct SegResult {
    int nk = 0, nheads = 0;
};

struct Chunk {
    mml_ctx* ctx;
    mml_ctx::BankCube& K;
    int i0, i1, nseg;
    MmlField<CubeSegDev> f_seg;
    MmlField<int> f_back, f_mbox;
    MmlField<char> f_grid;
    size_t up_bytes;
    Chunk(mml_ctx* c, int a, int b) : ctx(c), K(c->bank_cube), i0(a), i1(b), nseg(2 * (b - a)) {
        MmlCarve<16> carve;
        f_seg = carve.take<CubeSegDev>((size_t)nseg);
        f_back = carve.take<int>(4 * (size_t)nseg);
        f_mbox = carve.take<int>(6 * (size_t)nseg);
        up_bytes = carve.bytes();
        f_grid = carve.take<char>(mml_grid_table_bytes(nseg));
    }
    static size_t bytes(int nseg) {
        return sizeof(CubeSegDev) * (size_t)nseg + sizeof(int) * 10 * (size_t)nseg + mml_grid_table_bytes(nseg) + 16 * 8;
    }
    // the chunk's rows in the pinned twin (the match phase fills m_pts / m_tag / m_cnt in), the read-backs zeroed / emptied
    long long fill(MmlMapState* const* maps, const Move* mv, bool match) const {
        CubeSegDev* h = f_seg.in(K.tab.h);
        const int empty[6] = MML_BBOX_EMPTY;
        long long total = 0;
        for (int g = 0; g < nseg; ++g) {
            const int i = i0 + g / 2, kind = g & 1;
            const MmlCubeLive& L = maps[i]->clive;
            const MmlCubeMatch& G = maps[i]->cmatch;
            CubeSegDev& S = h[g];
            memset(static_cast<void*>(&S), 0, sizeof(S));
            S.spts = L.gs_pts[kind];
            S.stag = L.gs_tag[kind];
            S.out_pts = L.gs_pts2[kind];
            S.out_tag = L.gs_tag2[kind];
            S.ppts = L.gp_pts[kind];
            if (match) {
                S.m_pts = G.gmap_orig[kind];
                S.m_tag = G.gtag_orig[kind];
                S.m_cnt = G.cube_cnt[kind];
            }
            S.n0 = L.gs_n[kind];
            S.np = L.gp_n[kind];
            S.off = (int)total;
            total += S.n0 + S.np;
            for (int a = 0; a < 3; ++a) {
                S.cen[a] = mv[i].cen[a];
                S.up[a] = mv[i].up[a];
                S.down[a] = mv[i].down[a];
            }
            for (int c = 0; c < 6; ++c) f_mbox.in(K.tab.h)[6 * (size_t)g + c] = empty[c];
        }
        memset(f_back.in(K.tab.h), 0, f_back.bytes());
        return total;
    }
};

// the store chain of one chunk: writes scratch and the stores' second buffers only.  res: the call's 2 n results.
int chain_chunk(const Chunk& C, MmlMapState* const* maps, const Move* mv, SegResult* res) {
    mml_ctx* ctx = C.ctx;
    mml_ctx::BankCube& K = C.K;
    hipStream_t s = MML_STREAM(ctx);
    const int nseg = C.nseg;
    const long long total = C.fill(maps, mv, false);
    MML_REQUIRE(total <= (long long)K.cap && nseg <= K.seg_cap, MML_ERR_CAPACITY, "cube increment: more points than the scratch holds");
    if (total == 0) return MML_OK;  // (nothing stored, nothing pending: every size stays 0)
    const int P = (int)total;
    int max_nu = 0;
    const CubeSegDev* h_seg = C.f_seg.in(K.tab.h);
    for (int g = 0; g < nseg; ++g) max_nu = std::max(max_nu, h_seg[g].n0 + h_seg[g].np);
    MML_HIP(hipMemcpyAsync(K.tab.d, K.tab.h, C.up_bytes, hipMemcpyHostToDevice, s));
    const CubeSegDev* d_seg = C.f_seg.in(K.tab.d);
    int* d_back = C.f_back.in(K.tab.d);
    int* h_back = C.f_back.in(K.tab.h);
    int* cnt = K.work;
    int* changed = cnt + (size_t)nseg * NCUBE;
    int* bbox = changed + (size_t)nseg * NCUBE;
    int* keep = K.flags;
    int* keep_pos = keep + (K.cap + 1);
    int* sel = keep_pos + (K.cap + 1);
    int* sel_pos = sel + (K.cap + 1);
    unsigned long long* keys2 = K.keys + K.cap;
    unsigned* vals2 = K.vals + K.cap;
    uint16_t* tag = K.tags;
    uint16_t* sel_tag = K.tags + K.cap;
    const dim3 grid(blocks_for(max_nu), nseg);
    MML_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * 2 * (size_t)nseg * NCUBE, s));  // cnt + changed
    hipLaunchKernelGGL(k_cs_tag_hist, grid, dim3(256), 0, s, d_seg, tag, cnt, changed);
    hipLaunchKernelGGL(k_cs_classify, grid, dim3(256), 0, s, d_seg, tag, cnt, changed, keep, sel);
    int rc = mml_exclusive_scan(ctx, ctx->sort_tmp, keep, keep_pos, (size_t)P, s);
    if (rc == MML_OK) rc = mml_exclusive_scan(ctx, ctx->sort_tmp, sel, sel_pos, (size_t)P, s);
    if (rc != MML_OK) return rc;
    hipLaunchKernelGGL(k_cs_totals, dim3((nseg + 63) / 64), dim3(64), 0, s, d_seg, nseg, keep, keep_pos, sel, sel_pos, d_back);
    MML_HIP(hipMemcpyAsync(h_back, d_back, sizeof(int) * 2 * (size_t)nseg, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));  // read-back 1: the capacity decision
    long long nsel_total = 0;
    int max_sel = 0;
    for (int g = 0; g < nseg; ++g) {
        const int nk = h_back[g], nsel = h_back[nseg + g];
        if (nk + (long long)nsel > ctx->MM)
            return refuse_store(ctx, MML_ERR_CAPACITY, *maps[C.i0 + g / 2], "cube store larger than max_map_points");
        res[2 * (size_t)C.i0 + g].nk = nk;
        nsel_total += nsel;
        max_sel = std::max(max_sel, nsel);
    }
    hipLaunchKernelGGL(k_cs_init_bbox, dim3((unsigned)((6 * (size_t)nseg * NCUBE + 255) / 256)), dim3(256), 0, s, bbox, 6 * nseg * NCUBE);
    hipLaunchKernelGGL(k_cs_scatter, grid, dim3(256), 0, s, d_seg, tag, keep, keep_pos, sel, sel_pos, K.sel_pts, sel_tag, bbox);
    if (nsel_total) {
        const int NS = (int)nsel_total;
        const dim3 sgrid(blocks_for(max_sel), nseg);
        const float leaf = 0.4f;  // MAP_MANAGER's own filters, Map_Manager.cpp:58-60 (corner and surf alike)
        hipLaunchKernelGGL(k_cs_vox_keys, sgrid, dim3(256), 0, s, d_back, nseg, K.sel_pts, sel_tag, bbox, leaf, K.keys, K.vals);
        rc = mml_sort_pairs(ctx, ctx->sort_tmp, K.keys, keys2, K.vals, vals2, (size_t)NS, mml_cube_key_bits(nseg), s);
        if (rc != MML_OK) return rc;
        // keep / keep_pos are free again
        hipLaunchKernelGGL(k_run_heads<unsigned long long>, dim3((NS + 255) / 256), dim3(256), 0, s, keys2, NS, 0, ~0ull, keep);
        rc = mml_exclusive_scan(ctx, ctx->sort_tmp, keep, keep_pos, (size_t)NS, s);
        if (rc != MML_OK) return rc;
        hipLaunchKernelGGL(k_cs_centroid, sgrid, dim3(256), 0, s, d_seg, d_back, nseg, K.sel_pts, keys2, vals2, keep, keep_pos, ctx->MM);
        MML_HIP(hipMemcpyAsync(h_back + 3 * (size_t)nseg, d_back + 3 * (size_t)nseg, sizeof(int) * (size_t)nseg, hipMemcpyDeviceToHost, s));
        MML_HIP(hipStreamSynchronize(s));  // read-back 2: the filtered sizes
        for (int g = 0; g < nseg; ++g) res[2 * (size_t)C.i0 + g].nheads = h_back[3 * (size_t)nseg + g];
    }
    MML_HIP(hipGetLastError());
    return MML_OK;
}

// the match copies of one chunk, from the live arrays the chain has not touched: every capacity decision of the call has passed
int match_chunk(const Chunk& C, MmlMapState* const* maps, const Move* mv, int* rounds) {
    mml_ctx* ctx = C.ctx;
    mml_ctx::BankCube& K = C.K;
    hipStream_t s = MML_STREAM(ctx);
    const int nseg = C.nseg;
    int max_n0 = 0;
    bool grows = false;
    for (int g = 0; g < nseg; ++g) {
        const MmlMapState& M = *maps[C.i0 + g / 2];
        grows = grows || !mml_cube_match_fits(M.cmatch, g & 1, M.clive.gs_n[g & 1]);
    }
    if (grows) MML_HIP(hipStreamSynchronize(s));  // (a copy that has to grow is replaced with nothing in flight: at most one more wait)
    for (int g = 0; g < nseg; ++g) {
        MmlCubeMatch& G = maps[C.i0 + g / 2]->cmatch;
        const MmlCubeLive& L = maps[C.i0 + g / 2]->clive;
        const int kind = g & 1;
        G.have_gmap[kind] = false;
        for (int a = 0; a < 3; ++a) G.cen[a] = L.gs_cen[a];  // the centre BEFORE MapMove (laserCloudCen*_last)
        const int rc = mml_cube_match_ensure(ctx, G, kind, L.gs_n[kind]);
        if (rc != MML_OK) return rc;
        max_n0 = std::max(max_n0, L.gs_n[kind]);
    }
    ctx->banks.dirty = true;  // (the cube table of a context with banks holds a copy of these maps' rows)
    C.fill(maps, mv, true);
    MML_HIP(hipMemcpyAsync(K.tab.d, K.tab.h, C.up_bytes, hipMemcpyHostToDevice, s));
    const CubeSegDev* d_seg = C.f_seg.in(K.tab.d);
    int* d_mbox = C.f_mbox.in(K.tab.d);
    int* h_mbox = C.f_mbox.in(K.tab.h);
    hipLaunchKernelGGL(k_cs_zero_cnt, dim3((NCUBE + 255) / 256, nseg), dim3(256), 0, s, d_seg);
    if (max_n0) hipLaunchKernelGGL(k_cs_match_copy, dim3(blocks_for(max_n0), nseg), dim3(256), 0, s, d_seg, d_mbox);
    MML_HIP(hipMemcpyAsync(h_mbox, d_mbox, C.f_mbox.bytes(), hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));  // the bounding boxes of all match copies
    std::vector<MmlGridJob> jobs((size_t)nseg);
    for (int g = 0; g < nseg; ++g) {
        MmlCubeMatch& G = maps[C.i0 + g / 2]->cmatch;
        const int kind = g & 1;
        jobs[g] = MmlGridJob{&G.ggrid[kind], G.gmap_orig[kind], kind == 0 ? ctx->cfg.cell_corner : ctx->cfg.cell_surf,
                             maps[C.i0 + g / 2]->clive.gs_n[kind], h_mbox + 6 * (size_t)g, G.gtag_orig[kind]};
    }
    const MmlGridScratch<unsigned long long> W{K.keys, K.keys + K.cap, K.vals, K.vals + K.cap, K.cap, C.f_grid.in(K.tab.d), C.f_grid.in(K.tab.h)};
    const int rc = mml_build_grids(ctx, nseg, jobs.data(), W, rounds);
    if (rc != MML_OK) return rc;
    for (int g = 0; g < nseg; ++g) maps[C.i0 + g / 2]->cmatch.have_gmap[g & 1] = jobs[g].m > 0;
    return MML_OK;
}

}  // namespace

// The store's own memory (72 bytes x max_map_points + 2 x 16 x max_features x 16 bytes), allocated by the first call that needs it.
// The scratch the chain works in is the context's bank_cube, grown by the increment to the points it works on.
int mml_cube_store_ensure(mml_ctx* ctx, MmlMapState& map) {
    MmlCubeLive& L = map.clive;
    if (L.mem.present()) return MML_OK;
    const size_t MM = (size_t)ctx->MM;
    const size_t gp = 16 * (size_t)ctx->MF;
    L.gp_cap = (int)gp;
    return L.mem.reserve(
        ctx, {mml_part(L.gs_pts[0], MM), mml_part(L.gs_tag[0], MM), mml_part(L.gs_pts2[0], MM), mml_part(L.gs_tag2[0], MM), mml_part(L.gp_pts[0], gp),
              mml_part(L.gs_pts[1], MM), mml_part(L.gs_tag[1], MM), mml_part(L.gs_pts2[1], MM), mml_part(L.gs_tag2[1], MM), mml_part(L.gp_pts[1], gp)});
}

int mml_cube_store_reset(mml_ctx* ctx, MmlMapState& map) {
    MmlCubeLive& L = map.clive;
    L.gs_n[0] = L.gs_n[1] = 0;
    L.gp_n[0] = L.gp_n[1] = 0;
    L.gs_cen[0] = 10;
    L.gs_cen[1] = 5;
    L.gs_cen[2] = 10;
    return MML_OK;
}

// the LIVE store (tests / visualisation): points, cube index of every point, centre
int mml_cube_store_download(mml_ctx* ctx, const MmlMapState& map, int kind, float* xyz, int* cube, int capacity, int* n, int* cen) {
    const MmlCubeLive& L = map.clive;
    hipStream_t s = MML_STREAM(ctx);
    const int m = L.gs_pts[kind] ? L.gs_n[kind] : 0;
    *n = m;
    if (cen)
        for (int k = 0; k < 3; ++k) cen[k] = L.gs_cen[k];
    if (m == 0 || (!xyz && !cube)) return MML_OK;
    MML_REQUIRE(capacity >= m, MML_ERR_CAPACITY, "capacity below the store size");
    std::vector<float4> p((size_t)m);
    std::vector<uint16_t> t((size_t)m);
    MML_HIP(hipMemcpyAsync(p.data(), L.gs_pts[kind], sizeof(float4) * (size_t)m, hipMemcpyDeviceToHost, s));
    MML_HIP(hipMemcpyAsync(t.data(), L.gs_tag[kind], sizeof(uint16_t) * (size_t)m, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < m; ++i) {
        if (xyz) {
            xyz[3 * i] = p[i].x;
            xyz[3 * i + 1] = p[i].y;
            xyz[3 * i + 2] = p[i].z;
        }
        if (cube) cube[i] = t[i];
    }
    return MML_OK;
}

std::vector<int> mml_cube_chunks(int n, const long long* pts, long long budget, int max_stores) {
    std::vector<int> cut(1, 0);
    long long run = 0;
    for (int i = 0; i < n; ++i) {
        if (i > cut.back() && (run + pts[i] > budget || i - cut.back() >= max_stores)) {
            cut.push_back(i);
            run = 0;
        }
        run += pts[i];
    }
    cut.push_back(n);
    return cut;
}

int mml_cube_store_increment_segmented(mml_ctx* ctx, int n, MmlMapState* const* maps, const double* T_wl, int* n_corner, int* n_surf) {
    hipStream_t s = MML_STREAM(ctx);
    mml_ctx::BankCube& K = ctx->bank_cube;
    // MapMove of every store on a host copy of its centre: a pose outside the grid refuses the call before the device is touched
    std::vector<Move> mv((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int rc = plan_move(ctx, maps[i]->clive.gs_cen, T_wl + 16 * (size_t)i, mv[i]);
        if (rc != MML_OK) return refuse_store(ctx, rc, *maps[i], "pose far outside the cube grid");
    }
    // memory, all of it before the first launch: the stores (a first increment), the scratch of the largest chunk, its tables,
    // the temporary storage of the sorts and scans
    std::vector<long long> pts((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int rc = mml_cube_store_ensure(ctx, *maps[i]);
        if (rc != MML_OK) return rc;
        const MmlCubeLive& L = maps[i]->clive;
        pts[i] = (long long)L.gs_n[0] + L.gp_n[0] + L.gs_n[1] + L.gp_n[1];
    }
    const std::vector<int> cut = mml_cube_chunks(n, pts.data(), K.budget, MML_BANK_GLOBAL_CHUNK_BANKS);
    long long max_pts = 1;
    int max_stores = 1;
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        long long run = 0;
        for (int i = cut[c]; i < cut[c + 1]; ++i) run += pts[i];
        max_pts = std::max(max_pts, run);
        max_stores = std::max(max_stores, cut[c + 1] - cut[c]);
    }
    MML_REQUIRE(max_pts < (1ll << 31), MML_ERR_CAPACITY, "cube increment: a chunk's stores exceed 2^31 points");
    if ((size_t)max_pts > K.cap || 2 * max_stores > K.seg_cap || !K.mem.present()) {
        const size_t cap = std::max((size_t)max_pts, K.cap);
        const int seg_cap = std::max(2 * max_stores, K.seg_cap);
        K.cap = 0;
        K.seg_cap = 0;
        const int rc = K.mem.reserve(ctx, {mml_part(K.work, (size_t)seg_cap * SEG_INTS), mml_part(K.flags, 4 * (cap + 1)), mml_part(K.keys, 2 * cap),
                                           mml_part(K.vals, 2 * cap), mml_part(K.sel_pts, cap), mml_part(K.tags, 2 * cap)});
        if (rc != MML_OK) return rc;
        K.cap = cap;
        K.seg_cap = seg_cap;
    }
    {
        const int nseg = 2 * max_stores;
        int rc = K.tab.reserve(ctx, Chunk::bytes(nseg));
        if (rc != MML_OK) return rc;
        int seg_bits = 1;
        while ((1 << seg_bits) < nseg) ++seg_bits;
        const size_t a = mml_sort_pairs_bytes<unsigned long long>((size_t)max_pts, mml_cube_key_bits(nseg), s);
        const size_t b = mml_sort_pairs_bytes<unsigned long long>((size_t)max_pts, 32 + seg_bits, s);
        rc = ctx->sort_tmp.reserve(ctx, std::max(a, b));
        if (rc != MML_OK) return rc;
    }
    // the store chains of all chunks: every capacity decision is taken before a match copy, a buffer pair or a centre changes
    std::vector<SegResult> res(2 * (size_t)n);
    std::vector<Chunk> chunks;
    for (size_t c = 0; c + 1 < cut.size(); ++c) chunks.emplace_back(ctx, cut[c], cut[c + 1]);
    for (const Chunk& C : chunks) {
        const int rc = chain_chunk(C, maps, mv.data(), res.data());
        if (rc != MML_OK) return rc;
    }
    // the match copies: the stores as they are, with their centres before MapMove (Map_Manager.cpp:136-149)
    for (const Chunk& C : chunks) {
        int rounds = 0;
        const int rc = match_chunk(C, maps, mv.data(), &rounds);
        if (rc != MML_OK) return rc;
    }
    // the commit: the buffer pairs swapped, sizes, centres, the pending clouds emptied
    for (int i = 0; i < n; ++i) {
        MmlCubeLive& L = maps[i]->clive;
        for (int kind = 0; kind < 2; ++kind) {
            std::swap(L.gs_pts[kind], L.gs_pts2[kind]);
            std::swap(L.gs_tag[kind], L.gs_tag2[kind]);
            L.gs_n[kind] = res[2 * (size_t)i + kind].nk + res[2 * (size_t)i + kind].nheads;
            L.gp_n[kind] = 0;
        }
        for (int a = 0; a < 3; ++a) L.gs_cen[a] = mv[i].cen[a];
        if (n_corner) n_corner[i] = L.gs_n[0];
        if (n_surf) n_surf[i] = L.gs_n[1];
    }
    MML_HIP(hipGetLastError());
    return MML_OK;
}

int mml_cube_store_append_segmented(mml_ctx* ctx, int n, MmlMapState* const* maps, const int* slots, const double* T_wl) {
    hipStream_t s = MML_STREAM(ctx);
    mml_ctx::BankCube& K = ctx->bank_cube;
    // the stack sizes in one copy (the context's 2 B ints), those of the n slots checked before a store's pending clouds change
    std::vector<int> nf(2 * (size_t)n);
    {
        int* h = reinterpret_cast<int*>(mml_stage_alloc(ctx, (size_t)ctx->B + 1));  // pinned
        MML_HIP(hipMemcpyAsync(h, ctx->ft_n, sizeof(int) * 2 * (size_t)ctx->B, hipMemcpyDeviceToHost, s));
        MML_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i)
            for (int kind = 0; kind < 2; ++kind) nf[2 * (size_t)i + kind] = h[(size_t)kind * ctx->B + slots[i]];
    }
    for (int i = 0; i < n; ++i)
        for (int kind = 0; kind < 2; ++kind) {
            const int f = nf[2 * (size_t)i + kind];
            if (f < 0 || f > ctx->MF) return mml_refuse(ctx, MML_ERR_STATE, "slot %d holds no down-sampled feature stack", slots[i]);
            if (maps[i]->clive.gp_n[kind] + (long long)f > 16ll * ctx->MF)
                return refuse_store(ctx, MML_ERR_CAPACITY, *maps[i], "too many pending map points (16 x max_features)");
        }
    for (int i = 0; i < n; ++i) {
        const int rc = mml_cube_store_ensure(ctx, *maps[i]);
        if (rc != MML_OK) return rc;
    }
    const size_t nseg = 2 * (size_t)n;
    int rc = K.tab.reserve(ctx, sizeof(CubeAppDev) * nseg);
    if (rc != MML_OK) return rc;
    CubeAppDev* h = reinterpret_cast<CubeAppDev*>(K.tab.h);
    int max_n = 0;
    for (int i = 0; i < n; ++i) {
        MmlCubeLive& L = maps[i]->clive;
        for (int kind = 0; kind < 2; ++kind) {
            CubeAppDev& S = h[2 * (size_t)i + kind];
            memset(static_cast<void*>(&S), 0, sizeof(S));
            S.feat = ctx->ft_xyz[kind] + (size_t)slots[i] * ctx->MF;
            S.out = L.gp_pts[kind] + L.gp_n[kind];
            memcpy(S.T, T_wl + 16 * (size_t)i, sizeof(double) * 12);
            S.n = nf[2 * (size_t)i + kind];
            max_n = std::max(max_n, S.n);
        }
    }
    if (max_n) {
        MML_HIP(hipMemcpyAsync(K.tab.d, K.tab.h, sizeof(CubeAppDev) * nseg, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_cs_to_world, dim3(blocks_for(max_n), (unsigned)nseg), dim3(256), 0, s, reinterpret_cast<const CubeAppDev*>(K.tab.d));
        MML_HIP(hipGetLastError());
    }
    for (int i = 0; i < n; ++i)
        for (int kind = 0; kind < 2; ++kind) maps[i]->clive.gp_n[kind] += nf[2 * (size_t)i + kind];
    return MML_OK;
}
