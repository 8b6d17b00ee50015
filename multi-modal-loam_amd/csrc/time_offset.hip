// time_offset.hip -- SURVEY 8(f) rank 4 (part): the numeric core of LidarsParamEstimator::estimate_timeoffset
// (unionLidarsAligner.cpp:1077-1153) for n problems per call.
//   problem = one Velodyne FOV cloud (transformed by its own 4 x 4 float matrix), one merged Livox cloud:
//   :1080-1082  pcl::transformPointCloud of the Velodyne cloud                      k_tofs_tf
//   :1084-1103  squared distance of every Livox point to its nearest Velodyne point k_tofs_box .. k_tofs_nn1
//   :1111-1131  sliding-window error sums                                           k_tofs_window_err
//   :1107,1141-1150  first strict minimum below 1e6                                 k_tofs_best
// ONE set of kernels serves mml_time_offset_search and mml_time_offset_search_batch: every kernel reads a per-problem device
// table (TofsProb) with the problem index in blockIdx.y, and the single call is the n = 1 case.  A problem's arithmetic does
// not depend on the problems next to it: its distances come from an EXACT search (knn5_dev.h), which returns the same float
// whatever grid it walks, and its window sums are formed by one lane each in index order.
// mml_time_offset_estimate_stream is the whole of estimate_timeoffset (:1021-1166) on a resident mml_livox_stream: the FOV
// selection's stage (velo_fov.hip) feeds the same kernels on the device, k_tofs_livox_xyz forms the Livox side from the stream's
// records (one block shared by all frames: TofsProb::q_base) and k_tofs_rows turns the best windows into stamps (:1146, :1159-1161).
// The gate of :1026-1043 is host code: time_offset_gate.h.
// Compiled with -ffp-contract=off.
#include <math.h>
#include <string.h>

#include "mml_internal.h"
#include "time_offset_gate.h"
#include "voxel_sort_dev.h"

namespace {

#include "knn5_dev.h"

// One problem of a call.  Rows are counted from the call's first row (velo_offsets[0] / livox_offsets[0]); g.pts and g.cell_start
// point into the call's blocks and g is complete once the boxes have been read back (tofs_choose_grid).
struct TofsProb {
    MmlGrid g;
    int v_base, n_velo;
    int l_base, n_livox;  // its rows of the distance array
    long long e_base;     // first window of the problem in the error array
    int n_win;
    int q_base;  // its first Livox point in the query array: l_base, or 0 where all problems share one Livox block (the stream call)
};
struct TofsBest {
    double lowest;
    int best, _pad;
};

constexpr int TOFS_BOX_BLOCKS = 64;  // workgroups per problem of the bounding-box pass (each strides over the cloud)

// pcl::transformPointCloud (PCL 1.8.1 common/impl/transforms.hpp), float, left to right; tf == nullptr: copy
__global__ __launch_bounds__(256) void k_tofs_tf(const TofsProb* __restrict__ tab, const float* __restrict__ xyz, const float* __restrict__ tf,
                                                 float4* __restrict__ out) {
    const int base = tab[blockIdx.y].v_base, n = tab[blockIdx.y].n_velo;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* p = xyz + 3 * (size_t)(base + i);
    const float x = p[0], y = p[1], z = p[2];
    float4 o = make_float4(x, y, z, 0.f);
    if (tf) {
        const float* t = tf + 16 * (size_t)blockIdx.y;
        o.x = t[0] * x + t[1] * y + t[2] * z + t[3];
        o.y = t[4] * x + t[5] * y + t[6] * z + t[7];
        o.z = t[8] * x + t[9] * y + t[10] * z + t[11];
    }
    out[base + i] = o;
}

// bounding box of every problem's transformed cloud: box[6 p ..] = min xyz, max xyz as keys (the host uploads MML_BBOX_EMPTY)
__global__ __launch_bounds__(256) void k_tofs_box(const TofsProb* __restrict__ tab, const float4* __restrict__ pts, int* __restrict__ box) {
    const int base = tab[blockIdx.y].v_base, n = tab[blockIdx.y].n_velo;
    if ((int)blockIdx.x * 256 >= n) return;  // (the whole workgroup)
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float4 p = pts[base + i];
        mn[0] = fminf(mn[0], p.x);
        mn[1] = fminf(mn[1], p.y);
        mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x);
        mx[1] = fmaxf(mx[1], p.y);
        mx[2] = fmaxf(mx[2], p.z);
    }
    mml_bbox_block_reduce(mn, mx, box + 6 * (size_t)blockIdx.y);
}

// sort key of every point: problem << 32 | cell (the cell mapping of map_assoc.hip's k_grid_keys), value: its index in the problem
__global__ __launch_bounds__(256) void k_tofs_keys(const TofsProb* __restrict__ tab, const float4* __restrict__ pts,
                                                   unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
    const TofsProb& P = tab[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n_velo) return;
    const float4 p = pts[P.v_base + i];
    const float inv = P.g.inv_cell;
    const int dx = P.g.dim[0], dy = P.g.dim[1], dz = P.g.dim[2];
    const int cx = cell_coord(p.x, P.g.origin[0], inv, dx);
    const int cy = cell_coord(p.y, P.g.origin[1], inv, dy);
    const int cz = cell_coord(p.z, P.g.origin[2], inv, dz);
    keys[P.v_base + i] = ((unsigned long long)blockIdx.y << 32) | (unsigned)(cx + dx * (cy + dy * cz));
    vals[P.v_base + i] = (unsigned)i;
}

// The sort keeps a problem's points in its own rows (the problem is the key's high word and the rows were in problem order):
// sorted row v_base + i holds the problem's i-th point in cell order, w = its index in the problem's cloud.
__global__ __launch_bounds__(256) void k_tofs_gather(const TofsProb* __restrict__ tab, const float4* __restrict__ pts,
                                                     const unsigned* __restrict__ vals, float4* __restrict__ out) {
    const int base = tab[blockIdx.y].v_base, n = tab[blockIdx.y].n_velo;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned src = vals[base + i];
    float4 p = pts[base + src];
    p.w = __uint_as_float(src);
    out[base + i] = p;
}

// cell_start[c] = first sorted point of the problem whose cell >= c (lower bound); cell_start[ncell] = n_velo
__global__ __launch_bounds__(256) void k_tofs_cell_start(const TofsProb* __restrict__ tab, const unsigned long long* __restrict__ keys) {
    const TofsProb& P = tab[blockIdx.y];
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (P.n_velo == 0 || c > P.g.ncell) return;
    const unsigned long long* k = keys + P.v_base;
    int lo = 0, hi = P.n_velo;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned)k[mid] < (unsigned)c)
            lo = mid + 1;
        else
            hi = mid;
    }
    P.g.cell_start[c] = lo;
}

// :1084-1103 squared distance to the nearest neighbour (the exact 5-NN search, first entry).  A workgroup serves ONE problem, so
// its grid descriptor is wave-uniform: copied out of the table once, it stays in scalar registers (see k_associate, map_assoc.hip).
__global__ __launch_bounds__(256) void k_tofs_nn1(const TofsProb* __restrict__ tab, const float* __restrict__ q_all, float* __restrict__ d2_all) {
    const TofsProb& P = tab[blockIdx.y];
    const int nq = P.n_livox;
    if ((int)blockIdx.x * 256 >= nq) return;  // (the whole workgroup: knn5_search needs whole wavefronts)
    MmlGrid g;
    g.pts = P.g.pts;
    g.cell_start = P.g.cell_start;
    g.tags = nullptr;
    g.m = P.g.m;
    g.origin[0] = P.g.origin[0];
    g.origin[1] = P.g.origin[1];
    g.origin[2] = P.g.origin[2];
    g.cell = P.g.cell;
    g.inv_cell = P.g.inv_cell;
    g.dim[0] = P.g.dim[0];
    g.dim[1] = P.g.dim[1];
    g.dim[2] = P.g.dim[2];
    g.ncell = P.g.ncell;
    const float* q = q_all + 3 * (size_t)P.q_base;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < nq;
    Knn5 k;
    knn5_search(g, valid, valid ? q[3 * i] : 0.f, valid ? q[3 * i + 1] : 0.f, valid ? q[3 * i + 2] : 0.f, INFINITY, k);
    if (valid) d2_all[P.l_base + i] = knn_d(k, 0);
}

// :1111-1131 one lane per (problem, window), found through the exclusive scan of the window counts (woff, n + 1 entries);
// the terms are added in index order, in double, as the reference's loop does
__global__ __launch_bounds__(64) void k_tofs_window_err(const TofsProb* __restrict__ tab, int n, const long long* __restrict__ woff,
                                                        const float* __restrict__ q_all, const float* __restrict__ d2_all, int res, int sliced,
                                                        double* __restrict__ err) {
    const long long w = (long long)blockIdx.x * 64 + threadIdx.x;
    if (w >= woff[n]) return;
    int lo = 0, hi = n;  // the problem p with woff[p] <= w < woff[p + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (woff[mid] <= w)
            lo = mid;
        else
            hi = mid;
    }
    const TofsProb& P = tab[lo];
    const int cnt = (int)(w - woff[lo]);
    const float* q = q_all + 3 * (size_t)P.q_base;
    const float* d2 = d2_all + P.l_base;
    double sum_error = 0;
    for (int i = cnt * res; i < cnt * res + sliced; ++i) {
        const float x = q[3 * i], y = q[3 * i + 1];
        sum_error += d2[i] + 0.2 * sqrtf(x * x + y * y);
    }
    err[w] = sum_error;
}

// :1107,1141-1150 per problem: the lowest window error below 1e6 and the first window that has it (-1: none)
__device__ __forceinline__ void tofs_better(double& lo, int& best, double lo2, int best2) {
    if (lo2 < lo || (lo2 == lo && best2 >= 0 && best2 < best)) {
        lo = lo2;
        best = best2;
    }
}
__global__ __launch_bounds__(256) void k_tofs_best(const TofsProb* __restrict__ tab, const double* __restrict__ err, TofsBest* __restrict__ out) {
    __shared__ double s_lo[4];
    __shared__ int s_best[4];
    const TofsProb& P = tab[blockIdx.x];
    const double* e = err + P.e_base;
    double lo = 1000000.0;
    int best = -1;
    for (int c = threadIdx.x; c < P.n_win; c += 256) {  // (ascending in a lane: the first of equal values stays)
        const double v = e[c];
        if (v < lo) {
            lo = v;
            best = c;
        }
    }
    for (int o = 32; o > 0; o >>= 1) tofs_better(lo, best, __shfl_xor(lo, o), __shfl_xor(best, o));
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_best[threadIdx.x >> 6] = best;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) tofs_better(lo, best, s_lo[w], s_best[w]);
        out[blockIdx.x].lowest = lo;
        out[blockIdx.x].best = best;
    }
}

// ---- mml_time_offset_estimate_stream: the Livox side and the stamps come from a resident mml_livox_stream ---------------------

constexpr int TOFS_XYZ_BLOCKS = 1024;  // workgroups of k_tofs_livox_xyz at most (each strides over the output)

// The packed x, y, z of the stream records [rec, rec + 5 n): dwords 1 .. 3 of every 5-dword record (mml_livox_point).  Source and
// destination are walked as dword streams: consecutive lanes write consecutive dwords of `out` and read dwords that lie at most two
// apart, so a wave's 64 loads fall into the 107 consecutive dwords the 64 stores need -- every fetched line is used, and the 8 of
// 20 bytes per record that are not coordinates are the only excess.  Bit copies: no float operation touches a coordinate.
__global__ __launch_bounds__(256) void k_tofs_livox_xyz(const uint32_t* __restrict__ rec, long long n, uint32_t* __restrict__ out) {
    const long long nd = 3 * n;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < nd; o += (long long)gridDim.x * 256) {
        const long long k = o / 3;
        out[o] = rec[5 * k + 1 + (o - 3 * k)];
    }
}

// The rows of the stream call, one lane per frame: what the search found, the stamp of the best window's first point read from the
// stream's stamp array (S points at the range's first point; :1146), the offset (:1161) and the threshold (:1159).  A frame that
// kept nothing while the range holds points (range_points > 0) is NO_VELO_IN_FOV; its problem has no window, so best stays -1.
__global__ __launch_bounds__(64) void k_tofs_rows(const TofsProb* __restrict__ tab, const TofsBest* __restrict__ best, int n,
                                                  const uint64_t* __restrict__ S, uint64_t hs, int res, long long range_points,
                                                  const uint64_t* __restrict__ velo_stamps, double error_th,
                                                  mml_time_offset_estimate_row* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const TofsProb& P = tab[i];
    mml_time_offset_estimate_row r;
    r.status = (P.n_velo == 0 && range_points > 0) ? MML_TOFS_ROW_NO_VELO_IN_FOV : MML_TOFS_ROW_OK;
    r.n_kept = P.n_velo;
    r.n_windows = P.n_win;
    r.best_window = P.n_win > 0 ? best[i].best : -1;
    r.lowest_error = P.n_win > 0 ? best[i].lowest : 1000000.0;
    r.optim_start = 0;
    r.time_offset = 0;
    r.accepted = 0;
    r._pad = 0;
    if (r.best_window >= 0) {  // (best_window * res + sliced < range_points: the index lies inside the range)
        r.optim_start = hs + S[(long long)r.best_window * res];
        r.time_offset = velo_stamps[i] - r.optim_start;
        r.accepted = r.lowest_error < error_th ? 1 : 0;
    }
    out[i] = r;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// Why a call is refused (mml_time_offset_plan's checks, in this order); `bad`: the problem it is about, -1 when it is not about one.
enum { TOFS_OK = 0, TOFS_N, TOFS_NULL, TOFS_PARAM, TOFS_NEGATIVE, TOFS_DECREASING, TOFS_NO_VELO, TOFS_TOO_LARGE };
int tofs_plan(int n, const int* vo, const int* lo, int res, int sliced, int max_map_points, int* nwin, int* bad) {
    *bad = -1;
    if (n < 1 || n > MML_TOFS_BATCH_MAX) return TOFS_N;
    if (!vo || !lo) return TOFS_NULL;
    if (res < 1 || sliced < 1) return TOFS_PARAM;
    *bad = 0;
    if (vo[0] < 0 || lo[0] < 0) return TOFS_NEGATIVE;
    for (int i = 0; i < n; ++i)
        if (vo[i + 1] < vo[i] || lo[i + 1] < lo[i]) {
            *bad = i;
            return TOFS_DECREASING;
        }
    for (int i = 0; i < n; ++i) {
        const int nv = vo[i + 1] - vo[i], nl = lo[i + 1] - lo[i];
        *bad = i;
        if (nl > 0 && nv == 0) return TOFS_NO_VELO;
        if (max_map_points >= 0 && nv > max_map_points) return TOFS_TOO_LARGE;
    }
    *bad = -1;
    if (nwin)
        for (int i = 0; i < n; ++i) {  // windows: cnt = 0, 1, ... while cnt * res + sliced < n_livox
            const int nl = lo[i + 1] - lo[i];
            nwin[i] = nl > sliced ? (nl - sliced - 1) / res + 1 : 0;
        }
    return TOFS_OK;
}
int tofs_code(int why) { return why == TOFS_OK ? MML_OK : (why == TOFS_TOO_LARGE ? MML_ERR_CAPACITY : MML_ERR_INVALID); }

// Cells a problem of m Velodyne points may use; the pool of cell_start arrays is reserved for the sum of these before any launch.
long long tofs_cell_budget(int m) { return 8ll * m + 64; }

// The grid of one problem from its bounding box and point count alone -- no occupancy round trip: start from the 0.5 m cell of an
// unfiltered scan, grow it by 1.26 (a factor 2 in volume) until the box fits the budget, then halve it up to four times while
// the box still fits (a scan is a set of surfaces, most cells of its box are empty: the budget of 8 cells per point leaves an
// occupied cell a handful of points).  The distances do not depend on the choice (the search is exact), only the time does.
void tofs_choose_grid(const float* box, int m, MmlGrid& g) {
    const long long cap = tofs_cell_budget(m);
    const auto dims = [&](float cell, int* dim) {
        long long total = 1;
        for (int c = 0; c < 3; ++c) {
            const float ext = box[3 + c] - box[c];
            double d = isfinite(ext) ? floor((double)(ext / cell)) + 1.0 : 1.0;  // (a box with an infinite side: one cell across)
            if (!(d >= 1.0)) d = 1.0;
            if (d > 1048576.0) d = 1048576.0;  // (2^20 per axis: the product stays below 2^63)
            dim[c] = (int)d;
            total *= dim[c];
        }
        return total;
    };
    float cell = 0.5f;
    int dim[3];
    long long total = dims(cell, dim);
    while (total > cap) {  // (ends: a cell beyond the largest finite side leaves one cell)
        cell *= 1.26f;
        total = dims(cell, dim);
    }
    for (int round = 0; round < 4; ++round) {
        int d2[3];
        const long long t2 = dims(cell * 0.5f, d2);
        if (t2 > cap || t2 == total) break;
        cell *= 0.5f;
        total = t2;
        memcpy(dim, d2, sizeof(dim));
    }
    g.cell = cell;
    g.inv_cell = 1.0f / cell;
    for (int c = 0; c < 3; ++c) {
        g.origin[c] = box[c];
        g.dim[c] = dim[c];
    }
    g.ncell = (int)total;
}

// io block (device + pinned twin): what crosses the bus in small pieces, and the window errors
struct TofsIo {
    MmlCarve<256> c;
    MmlField<TofsProb> tab;
    MmlField<float> tf;
    MmlField<int> box;  // six keys per problem (mml_fkey)
    MmlField<long long> woff;
    MmlField<TofsBest> best;
    MmlField<double> err;
    MmlField<uint64_t> vstamps;                 // the stream call only (n_rows = n, else 0): the frames' header stamps ...
    MmlField<mml_time_offset_estimate_row> rows;  // ... and its result rows
    size_t bytes;
    TofsIo(size_t n, size_t n_win, size_t n_rows = 0)
        : tab(c.take<TofsProb>(n)), tf(c.take<float>(16 * n)), box(c.take<int>(6 * n)), woff(c.take<long long>(n + 1)), best(c.take<TofsBest>(n)),
          err(c.take<double>(n_win)), vstamps(c.take<uint64_t>(n_rows)), rows(c.take<mml_time_offset_estimate_row>(n_rows)), bytes(c.bytes()) {}
};
// big block (device only): 100 bytes per Velodyne point (cells included), 16 per Livox point, the sort's scratch
struct TofsBig {
    MmlCarve<256> c;
    MmlField<float> vxyz;
    MmlField<float4> v4, pts;
    MmlField<unsigned long long> keys, keys2;
    MmlField<unsigned> vals, vals2;
    MmlField<float> lxyz, nn;
    MmlField<int> cells;
    MmlField<char> sort;
    size_t bytes;
    // nq: Livox points in the query array, nd: distances (= nq unless the problems share one Livox block)
    TofsBig(size_t nv, size_t nq, size_t nd, size_t n_cells, size_t sort_bytes)
        : vxyz(c.take<float>(3 * nv)), v4(c.take<float4>(nv)), pts(c.take<float4>(nv)), keys(c.take<unsigned long long>(nv)),
          keys2(c.take<unsigned long long>(nv)), vals(c.take<unsigned>(nv)), vals2(c.take<unsigned>(nv)), lxyz(c.take<float>(3 * nq)),
          nn(c.take<float>(nd)), cells(c.take<int>(n_cells)), sort(c.take<char>(sort_bytes)), bytes(c.bytes()) {}
};

int bits_for(long long values) {  // bits that hold 0 .. values - 1
    int bits = 1;
    while ((1ll << bits) < values) ++bits;
    return bits;
}

// Every problem's cell and dims from the boxes that were read back, in one pass; its cell_start array follows the previous
// problem's in the pool.  Returns the largest cell count.
int tofs_lay_out_grids(int n, TofsProb* h_tab, const int* h_box, float4* d_pts, int* d_cells) {
    size_t cell_at = 0;
    int max_cells = 0;
    for (int i = 0; i < n; ++i) {
        TofsProb& P = h_tab[i];
        if (P.n_velo == 0) continue;
        float box[6];
        for (int c = 0; c < 6; ++c) box[c] = mml_funkey(h_box[6 * i + c]);
        tofs_choose_grid(box, P.n_velo, P.g);
        P.g.m = P.n_velo;
        P.g.pts = d_pts + P.v_base;
        P.g.cell_start = d_cells + cell_at;
        cell_at += (size_t)P.g.ncell + 1;
        max_cells = P.g.ncell > max_cells ? P.g.ncell : max_cells;
    }
    return max_cells;
}

// The box stage behind the uploads of the clouds (and of the matrices, with_tf): table, empty boxes and window offsets go down out
// of the pinned block h, the transform and the box pass run, the boxes come back -- and the stage's host synchronisation.
int tofs_finish_box(mml_ctx* ctx, int n, const TofsIo& io, const TofsBig& big, char* h, char* g, char* b, int max_v, bool with_tf) {
    hipStream_t s = MML_STREAM(ctx);
    const TofsProb* d_tab = io.tab.in(g);
    float4* d_v4 = big.v4.in(b);
    const unsigned by = (unsigned)n, bx_v = (unsigned)((max_v + 255) / 256);
    MML_HIP(hipMemcpyAsync(io.tab.in(g), io.tab.in(h), io.tab.bytes(), hipMemcpyHostToDevice, s));
    MML_HIP(hipMemcpyAsync(io.box.in(g), io.box.in(h), io.box.bytes(), hipMemcpyHostToDevice, s));
    MML_HIP(hipMemcpyAsync(io.woff.in(g), io.woff.in(h), io.woff.bytes(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_tofs_tf, dim3(bx_v, by), dim3(256), 0, s, d_tab, big.vxyz.in(b), with_tf ? io.tf.in(g) : nullptr, d_v4);
    hipLaunchKernelGGL(k_tofs_box, dim3(bx_v < (unsigned)TOFS_BOX_BLOCKS ? bx_v : (unsigned)TOFS_BOX_BLOCKS, by), dim3(256), 0, s, d_tab, d_v4,
                       io.box.in(g));
    MML_HIP(hipGetLastError());
    MML_HIP(hipMemcpyAsync(io.box.in(h), io.box.in(g), io.box.bytes(), hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    return MML_OK;
}

// The launches of the search stage: the finished table (pinned block h) goes down again, then keys, the sort, the gather, the
// cell starts, the distances and -- with a window in the call -- the window errors and every problem's best one.
int tofs_enqueue_search(mml_ctx* ctx, int n, const TofsIo& io, const TofsBig& big, char* h, char* g, char* b, size_t nv, size_t sort_bytes,
                        int max_v, int max_l, int max_cells, size_t n_win, int res, int sliced) {
    hipStream_t s = MML_STREAM(ctx);
    const TofsProb* d_tab = io.tab.in(g);
    float4 *d_v4 = big.v4.in(b), *d_pts = big.pts.in(b);
    unsigned long long *d_keys = big.keys.in(b), *d_keys2 = big.keys2.in(b);
    unsigned *d_vals = big.vals.in(b), *d_vals2 = big.vals2.in(b);
    const float* d_lxyz = big.lxyz.in(b);
    float* d_nn = big.nn.in(b);
    const unsigned by = (unsigned)n, bx_v = (unsigned)((max_v + 255) / 256);
    MML_HIP(hipMemcpyAsync(io.tab.in(g), io.tab.in(h), io.tab.bytes(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_tofs_keys, dim3(bx_v, by), dim3(256), 0, s, d_tab, d_v4, d_keys, d_vals);
    // ONE stable sort over all Velodyne points; with one problem the high word is zero and the cell bits are enough
    const int end_bit = n == 1 ? bits_for(max_cells) : 32 + bits_for(n);
    MmlTmpSpan sort_tmp{big.sort.in(b), sort_bytes};  // (carved out of the big block: nothing is allocated between the launches)
    const int rc = mml_sort_pairs(ctx, sort_tmp, d_keys, d_keys2, d_vals, d_vals2, nv, end_bit, s);
    if (rc != MML_OK) return rc;
    hipLaunchKernelGGL(k_tofs_gather, dim3(bx_v, by), dim3(256), 0, s, d_tab, d_v4, d_vals2, d_pts);
    hipLaunchKernelGGL(k_tofs_cell_start, dim3((unsigned)((max_cells + 1 + 255) / 256), by), dim3(256), 0, s, d_tab, d_keys2);
    hipLaunchKernelGGL(k_tofs_nn1, dim3((unsigned)((max_l + 255) / 256), by), dim3(256), 0, s, d_tab, d_lxyz, d_nn);
    if (n_win > 0) {
        hipLaunchKernelGGL(k_tofs_window_err, dim3((unsigned)((n_win + 63) / 64)), dim3(64), 0, s, d_tab, n, io.woff.in(g), d_lxyz, d_nn, res,
                           sliced, io.err.in(g));
        hipLaunchKernelGGL(k_tofs_best, dim3(by), dim3(256), 0, s, d_tab, io.err.in(g), io.best.in(g));
    }
    MML_HIP(hipGetLastError());
    return MML_OK;
}

}  // namespace

// Grow-only scratch of the time-offset searches, owned by the context: nothing is allocated or freed per call once the largest
// call has been seen.  Every entry point drains the stream before it returns, so reserve() never replaces a buffer in use.
struct MmlTofsDev {
    MmlStaging<char> io;
    MmlStaging<char, false> big;
    ~MmlTofsDev() {
        io.release();
        big.release();
    }
};

namespace {

// The n searches of mml_time_offset_search_batch; mml_time_offset_search is its n = 1 case.  `who`: the entry point the caller
// used, which is the name a refusal carries.  Every refusal comes before any device work and before any output is written.
int tofs_run(mml_ctx* ctx, const char* who, int n, const float* velo_xyz, const int* vo, const float* tf, const float* livox_xyz, const int* lo,
             int res, int sliced, float* nn_d2, double* window_error, const long* wo, int* n_windows, int* best_window, double* lowest_error) {
    std::vector<int> nwin((size_t)(n > 0 && n <= MML_TOFS_BATCH_MAX ? n : 1));
    int bad = -1;
    const int why = tofs_plan(n, vo, lo, res, sliced, ctx->MM, nwin.data(), &bad);
    switch (why) {
        case TOFS_N: return mml_refuse(ctx, MML_ERR_INVALID, "%s: n = %d is outside 1 .. %d", who, n, MML_TOFS_BATCH_MAX);
        case TOFS_NULL: return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null argument", who);
        case TOFS_PARAM: return mml_refuse(ctx, MML_ERR_INVALID, "%s: search_resolution / sliced_points must be >= 1", who);
        case TOFS_NEGATIVE: return mml_refuse(ctx, MML_ERR_INVALID, "%s: problem 0: a negative offset", who);
        case TOFS_DECREASING:
            return mml_refuse(ctx, MML_ERR_INVALID, "%s: problem %d: its clouds end before their start (offsets must not decrease)", who, bad);
        case TOFS_NO_VELO:
            return mml_refuse(ctx, MML_ERR_INVALID, "%s: problem %d: nearest-neighbour search in an empty cloud (Livox points, no Velodyne point)", who,
                              bad);
        case TOFS_TOO_LARGE:
            return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: problem %d: its Velodyne cloud of %d points exceeds max_map_points = %d", who, bad,
                              vo[bad + 1] - vo[bad], ctx->MM);
        default: break;
    }
    if (!(n_windows && best_window && lowest_error) || (window_error && !wo)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null argument", who);
    if (window_error) {
        if (wo[0] < 0) return mml_refuse(ctx, MML_ERR_INVALID, "%s: problem 0: a negative window offset", who);
        for (int i = 0; i < n; ++i)
            if (wo[i + 1] < wo[i]) return mml_refuse(ctx, MML_ERR_INVALID, "%s: problem %d: window offsets must not decrease", who, i);
    }
    const size_t nv = (size_t)(vo[n] - vo[0]), nl = (size_t)(lo[n] - lo[0]);
    if ((nv > 0 && !velo_xyz) || (nl > 0 && !livox_xyz)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null cloud", who);

    // Everything the context has in flight ends here -- every lane of a pipelined mml_step and the upload stream --, so a search that
    // follows a multi-lane step starts on an idle device; it reads no slot anyway: all it touches is the caller's arrays and its own block.
    int rc = mml_enter_idle(ctx);
    if (rc != MML_OK) return rc;

    size_t n_win = 0, n_cells = 0;
    int max_v = 0, max_l = 0;
    for (int i = 0; i < n; ++i) {
        const int m = vo[i + 1] - vo[i], l = lo[i + 1] - lo[i];
        n_win += (size_t)nwin[i];
        if (m > 0) n_cells += (size_t)tofs_cell_budget(m) + 1;
        max_v = m > max_v ? m : max_v;
        max_l = l > max_l ? l : max_l;
    }
    std::vector<TofsBest> best((size_t)n, TofsBest{1000000.0, -1, 0});
    const double* h_err = nullptr;
    if (nl > 0) {  // (no Livox point in the whole call: nothing to search)
        const size_t sort_bytes = mml_sort_pairs_bytes<unsigned long long>(nv, 64, MML_STREAM(ctx));
        const TofsIo io((size_t)n, n_win);
        const TofsBig big(nv, nl, nl, n_cells, sort_bytes);
        MmlTofsDev* d = mml_side<MmlTofsDev>(ctx, MML_SIDE_TIME_OFFSET);
        if (d->io.reserve(ctx, io.bytes) || d->big.reserve(ctx, big.bytes)) {
            ctx->err = std::string(who) + ": the scratch block could not be grown: " + ctx->err;
            return MML_ERR_HIP;
        }
        hipStream_t s = MML_STREAM(ctx);
        char *h = d->io.h, *g = d->io.d, *b = d->big.d;
        TofsProb* h_tab = io.tab.in(h);
        int* h_box = io.box.in(h);
        const int empty_box[6] = MML_BBOX_EMPTY;
        long long* h_woff = io.woff.in(h);
        h_woff[0] = 0;
        for (int i = 0; i < n; ++i) {
            TofsProb& P = h_tab[i];
            P = TofsProb{};
            P.v_base = vo[i] - vo[0];
            P.n_velo = vo[i + 1] - vo[i];
            P.l_base = P.q_base = lo[i] - lo[0];
            P.n_livox = lo[i + 1] - lo[i];
            P.e_base = h_woff[i];
            P.n_win = nwin[i];
            h_woff[i + 1] = h_woff[i] + nwin[i];
            memcpy(h_box + 6 * i, empty_box, sizeof(empty_box));
        }
        {   // host synchronisation 1 of 2: the boxes of all problems in one copy
            MmlStageScope t(ctx, "tofs_box");
            if (tf) MML_HIP(hipMemcpyAsync(io.tf.in(g), tf, io.tf.bytes(), hipMemcpyHostToDevice, s));
            MML_HIP(hipMemcpyAsync(big.vxyz.in(b), velo_xyz + 3 * (size_t)vo[0], big.vxyz.bytes(), hipMemcpyHostToDevice, s));
            MML_HIP(hipMemcpyAsync(big.lxyz.in(b), livox_xyz + 3 * (size_t)lo[0], big.lxyz.bytes(), hipMemcpyHostToDevice, s));
            rc = tofs_finish_box(ctx, n, io, big, h, g, b, max_v, tf != nullptr);
            if (rc != MML_OK) return rc;
        }
        const int max_cells = tofs_lay_out_grids(n, h_tab, h_box, big.pts.in(b), big.cells.in(b));
        {   // host synchronisation 2 of 2: the results
            MmlStageScope t(ctx, "tofs_search");
            rc = tofs_enqueue_search(ctx, n, io, big, h, g, b, nv, sort_bytes, max_v, max_l, max_cells, n_win, res, sliced);
            if (rc != MML_OK) return rc;
            if (n_win > 0) {
                MML_HIP(hipMemcpyAsync(io.best.in(h), io.best.in(g), io.best.bytes(), hipMemcpyDeviceToHost, s));
                if (window_error) MML_HIP(hipMemcpyAsync(io.err.in(h), io.err.in(g), io.err.bytes(), hipMemcpyDeviceToHost, s));
            }
            if (nn_d2) MML_HIP(hipMemcpyAsync(nn_d2 + lo[0], big.nn.in(b), sizeof(float) * nl, hipMemcpyDeviceToHost, s));
            MML_HIP(hipStreamSynchronize(s));
        }
        if (n_win > 0) {
            memcpy(best.data(), io.best.in(h), io.best.bytes());
            h_err = io.err.in(h);
        }
    }
    long long e_base = 0;
    for (int i = 0; i < n; ++i) {
        n_windows[i] = nwin[i];
        best_window[i] = best[i].best;
        lowest_error[i] = best[i].lowest;
        if (window_error && h_err && nwin[i] > 0) {  // at most the room the caller gave this problem
            const long room = wo[i + 1] - wo[i];
            const long k = room < (long)nwin[i] ? room : (long)nwin[i];
            if (k > 0) memcpy(window_error + wo[i], h_err + e_base, sizeof(double) * (size_t)k);
        }
        e_base += nwin[i];
    }
    return MML_OK;
}

// mml_time_offset_estimate_stream.  Every check that needs no device result comes before anything is enqueued and before any
// output is written; the one condition only the device knows -- a frame that keeps nothing -- becomes that row's status.
int tofs_stream_run(mml_ctx* ctx, mml_livox_stream* stream, long begin, long end, int n, const uint8_t* data, const long* byte_offsets,
                    const int* n_points, int step, int ox, int oy, int oz, const uint64_t* velo_stamps, const float* tf, int res, int sliced,
                    double error_th, float* nn_d2, double* window_error, const long* wo, mml_time_offset_estimate_row* out) {
    const char* who = "mml_time_offset_estimate_stream";
    const int n_max = MML_FOV_BATCH_MAX < MML_TOFS_BATCH_MAX ? MML_FOV_BATCH_MAX : MML_TOFS_BATCH_MAX;
    int rc = mml_vfov_check(ctx, who, n, n_max, data, byte_offsets, n_points, step, ox, oy, oz);
    if (rc != MML_OK) return rc;
    if (!stream || !velo_stamps || !out || (window_error && !wo)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null argument", who);
    const MmlLivoxView view = mml_livox_stream_view(stream);
    if (view.ctx != ctx) return mml_refuse(ctx, MML_ERR_INVALID, "%s: the stream belongs to another context", who);
    if (res < 1 || sliced < 1) return mml_refuse(ctx, MML_ERR_INVALID, "%s: search_resolution / sliced_points must be >= 1", who);
    if (!(view.front <= begin && begin <= end && end <= view.tail))
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: the range [%ld, %ld) is not inside the stream's live points [%ld, %ld)", who, begin, end,
                          view.front, view.tail);
    if (window_error) {
        if (wo[0] < 0) return mml_refuse(ctx, MML_ERR_INVALID, "%s: frame 0: a negative window offset", who);
        for (int i = 0; i < n; ++i)
            if (wo[i + 1] < wo[i]) return mml_refuse(ctx, MML_ERR_INVALID, "%s: frame %d: window offsets must not decrease", who, i);
    }
    const long long L = end - begin;
    long long total_in = 0;
    for (int i = 0; i < n; ++i) {  // (points, not kept points: what a frame keeps is known on the device only)
        if (n_points[i] > ctx->MM)
            return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: frame %d: its %d points exceed max_map_points = %d", who, i, n_points[i], ctx->MM);
        total_in += n_points[i];
    }
    if (total_in > 0x7fffffffll || (long long)n * L > 0x7fffffffll)
        return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: %lld Velodyne points or %d x %lld distances exceed INT_MAX", who, total_in, n, L);

    rc = mml_enter_idle(ctx);  // (the pushes still in flight on the stream end here too)
    if (rc != MML_OK) return rc;
    const mml_velo_fov_info* info = nullptr;  // host synchronisation 1 of 3: the FOV counts
    rc = mml_vfov_select_device(ctx, who, n, data, byte_offsets, n_points, step, ox, oy, oz, &info);
    if (rc != MML_OK) return rc;
    std::vector<long long> dst((size_t)n);
    std::vector<int> kept((size_t)n);
    size_t nv = 0, n_win = 0, n_cells = 0;
    int max_v = 0;
    const int nwin_each = L > sliced ? (int)((L - sliced - 1) / res) + 1 : 0;  // windows: cnt = 0, 1, ... while cnt * res + sliced < L
    for (int i = 0; i < n; ++i) {
        const int m = info[i].n_kept;
        kept[(size_t)i] = m;
        dst[(size_t)i] = (long long)nv;
        nv += (size_t)m;
        if (m > 0) {
            n_win += (size_t)nwin_each;
            n_cells += (size_t)tofs_cell_budget(m) + 1;
        }
        max_v = m > max_v ? m : max_v;
    }
    if (L == 0 || nv == 0) {  // nothing to search: an empty range, or no frame kept a point
        for (int i = 0; i < n; ++i)
            out[i] = mml_time_offset_estimate_row{L > 0 ? MML_TOFS_ROW_NO_VELO_IN_FOV : MML_TOFS_ROW_OK, kept[(size_t)i], 0, -1, 1000000.0, 0, 0, 0, 0};
        return MML_OK;
    }

    const size_t sort_bytes = mml_sort_pairs_bytes<unsigned long long>(nv, 64, MML_STREAM(ctx));
    const TofsIo io((size_t)n, n_win, (size_t)n);
    const TofsBig big(nv, (size_t)L, (size_t)n * (size_t)L, n_cells, sort_bytes);
    MmlTofsDev* d = mml_side<MmlTofsDev>(ctx, MML_SIDE_TIME_OFFSET);
    if (d->io.reserve(ctx, io.bytes) || d->big.reserve(ctx, big.bytes)) {
        ctx->err = std::string(who) + ": the scratch block could not be grown: " + ctx->err;
        return MML_ERR_HIP;
    }
    hipStream_t s = MML_STREAM(ctx);
    char *h = d->io.h, *g = d->io.d, *b = d->big.d;
    TofsProb* h_tab = io.tab.in(h);
    int* h_box = io.box.in(h);
    const int empty_box[6] = MML_BBOX_EMPTY;
    long long* h_woff = io.woff.in(h);
    h_woff[0] = 0;
    for (int i = 0; i < n; ++i) {
        const int m = kept[(size_t)i];
        TofsProb& P = h_tab[i];
        P = TofsProb{};
        P.v_base = (int)dst[(size_t)i];
        P.n_velo = m;
        P.l_base = (int)(i * L);  // (row i of the distances; all frames read the one Livox block at q_base = 0)
        P.n_livox = m > 0 ? (int)L : 0;
        P.e_base = h_woff[i];
        P.n_win = m > 0 ? nwin_each : 0;
        h_woff[i + 1] = h_woff[i] + P.n_win;
        memcpy(h_box + 6 * i, empty_box, sizeof(empty_box));
        if (tf) memcpy(io.tf.in(h) + 16 * (size_t)i, tf, sizeof(float) * 16);
    }
    memcpy(io.vstamps.in(h), velo_stamps, io.vstamps.bytes());
    const long at = begin - view.base;  // the range's first point in the live arrays
    {   // host synchronisation 2 of 3: the boxes
        MmlStageScope t(ctx, "tofs_box");
        if (tf) MML_HIP(hipMemcpyAsync(io.tf.in(g), io.tf.in(h), io.tf.bytes(), hipMemcpyHostToDevice, s));
        MML_HIP(hipMemcpyAsync(io.vstamps.in(g), io.vstamps.in(h), io.vstamps.bytes(), hipMemcpyHostToDevice, s));
        rc = mml_vfov_pack_device(ctx, n, dst.data(), max_v, big.vxyz.in(b));  // the FOV rows, device to device
        if (rc != MML_OK) return rc;
        const long long blocks = (3 * L + 255) / 256;
        hipLaunchKernelGGL(k_tofs_livox_xyz, dim3((unsigned)(blocks < TOFS_XYZ_BLOCKS ? blocks : TOFS_XYZ_BLOCKS)), dim3(256), 0, s,
                           view.rec + 5 * (size_t)at, L, reinterpret_cast<uint32_t*>(big.lxyz.in(b)));
        rc = tofs_finish_box(ctx, n, io, big, h, g, b, max_v, tf != nullptr);
        if (rc != MML_OK) return rc;
    }
    const int max_cells = tofs_lay_out_grids(n, h_tab, h_box, big.pts.in(b), big.cells.in(b));
    {   // host synchronisation 3 of 3: the rows
        MmlStageScope t(ctx, "tofs_search");
        rc = tofs_enqueue_search(ctx, n, io, big, h, g, b, nv, sort_bytes, max_v, (int)L, max_cells, n_win, res, sliced);
        if (rc != MML_OK) return rc;
        hipLaunchKernelGGL(k_tofs_rows, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, io.tab.in(g), io.best.in(g), n, view.stamp + at, view.hs, res,
                           L, io.vstamps.in(g), error_th, io.rows.in(g));
        MML_HIP(hipGetLastError());
        MML_HIP(hipMemcpyAsync(io.rows.in(h), io.rows.in(g), io.rows.bytes(), hipMemcpyDeviceToHost, s));
        if (window_error && n_win > 0) MML_HIP(hipMemcpyAsync(io.err.in(h), io.err.in(g), io.err.bytes(), hipMemcpyDeviceToHost, s));
        if (nn_d2)  // the rows of the frames that searched, runs of neighbours in one copy; a NO_VELO_IN_FOV row stays unwritten
            for (int i = 0; i < n;) {
                if (kept[(size_t)i] == 0) {
                    ++i;
                    continue;
                }
                int j = i;
                while (j < n && kept[(size_t)j] > 0) ++j;
                MML_HIP(hipMemcpyAsync(nn_d2 + (size_t)i * (size_t)L, big.nn.in(b) + (size_t)i * (size_t)L, sizeof(float) * (size_t)(j - i) * (size_t)L,
                                       hipMemcpyDeviceToHost, s));
                i = j;
            }
        MML_HIP(hipStreamSynchronize(s));
    }
    memcpy(out, io.rows.in(h), io.rows.bytes());
    if (window_error && n_win > 0) {
        const double* h_err = io.err.in(h);
        for (int i = 0; i < n; ++i) {  // at most the room the caller gave this frame
            const long room = wo[i + 1] - wo[i], have = h_tab[i].n_win;
            const long k = room < have ? room : have;
            if (k > 0) memcpy(window_error + wo[i], h_err + h_tab[i].e_base, sizeof(double) * (size_t)k);
        }
    }
    return MML_OK;
}

}  // namespace

extern "C" int mml_time_offset_estimate_stream(mml_ctx* ctx, mml_livox_stream* s, long livox_begin, long livox_end, int n, const uint8_t* data,
                                               const long* byte_offsets, const int* n_points, int point_step, int off_x, int off_y, int off_z,
                                               const uint64_t* velo_stamps, const float* tf, int search_resolution, int sliced_points,
                                               double error_th, float* nn_d2, double* window_error, const long* window_offsets,
                                               mml_time_offset_estimate_row* out) {
    if (!ctx) return MML_ERR_INVALID;
    return tofs_stream_run(ctx, s, livox_begin, livox_end, n, data, byte_offsets, n_points, point_step, off_x, off_y, off_z, velo_stamps, tf,
                           search_resolution, sliced_points, error_th, nn_d2, window_error, window_offsets, out);
}

extern "C" int mml_time_offset_gate(int n_velo, const uint64_t* velo_stamps, uint64_t hori_stamp, int n_hori_msgs, int* selected, int* status) {
    return time_offset_gate(n_velo, velo_stamps, hori_stamp, n_hori_msgs, selected, status);
}

extern "C" int mml_time_offset_plan(int n, const int* velo_offsets, const int* livox_offsets, int search_resolution, int sliced_points,
                                    int max_map_points, int* n_windows, int* bad_problem) {
    int bad = -1;
    const int why = tofs_plan(n, velo_offsets, livox_offsets, search_resolution, sliced_points, max_map_points, n_windows, &bad);
    if (bad_problem) *bad_problem = bad;
    return tofs_code(why);
}

extern "C" int mml_time_offset_search_batch(mml_ctx* ctx, int n, const float* velo_xyz, const int* velo_offsets, const float* tf,
                                            const float* livox_xyz, const int* livox_offsets, int search_resolution, int sliced_points,
                                            float* nn_d2, double* window_error, const long* window_offsets, int* n_windows, int* best_window,
                                            double* lowest_error) {
    if (!ctx) return MML_ERR_INVALID;
    return tofs_run(ctx, "mml_time_offset_search_batch", n, velo_xyz, velo_offsets, tf, livox_xyz, livox_offsets, search_resolution, sliced_points,
                    nn_d2, window_error, window_offsets, n_windows, best_window, lowest_error);
}

extern "C" int mml_time_offset_search(mml_ctx* ctx, const float* velo_xyz, int n_velo, const float* tf, const float* livox_xyz, int n_livox,
                                      int search_resolution, int sliced_points, float* nn_d2, double* window_error, int capacity, int* n_windows,
                                      int* best_window, double* lowest_error) {
    if (!ctx) return MML_ERR_INVALID;
    MML_REQUIRE(n_velo >= 0 && n_livox >= 0 && (n_velo == 0 || velo_xyz) && (n_livox == 0 || livox_xyz), MML_ERR_INVALID,
                "bad point buffers");
    MML_REQUIRE(search_resolution >= 1 && sliced_points >= 1, MML_ERR_INVALID, "search_resolution / sliced_points must be >= 1");
    MML_REQUIRE(n_windows && best_window && lowest_error, MML_ERR_INVALID, "null output");
    MML_REQUIRE(n_velo <= ctx->MM, MML_ERR_CAPACITY, "Velodyne cloud exceeds max_map_points");
    MML_REQUIRE(n_velo > 0 || n_livox == 0, MML_ERR_INVALID, "nearest-neighbour search in an empty cloud");
    const int vo[2] = {0, n_velo}, lo[2] = {0, n_livox};
    const long wo[2] = {0, capacity > 0 ? capacity : 0};
    return tofs_run(ctx, "mml_time_offset_search", 1, velo_xyz, vo, tf, livox_xyz, lo, search_resolution, sliced_points, nn_d2, window_error, wo,
                    n_windows, best_window, lowest_error);
}
