// map_assoc.hip -- rows a11..a16 of SURVEY.md section 8.
//   map side  : radix-sorted uniform grid over laserCloud{Corner,Surf}FromLocal -- replaces the
//               pcl::KdTreeFLANN::setInputCloud rebuild at mm-loam/src/lio/Estimator.cpp:1159-1167.
//   a13       : exact 5-NN (FLANN L2_Simple<float> semantics: d2 = ((dx*dx + dy*dy) + dz*dz) in float,
//               ascending, ties by lower index), one query per lane, ring-expanding cell search with an
//               exactness bound (all points within r*cell + margin are visited before stopping).
//   a11/a14/a15/a16 : pointAssociateToMap (Map_Manager.cpp:75-89), line fit (Estimator.cpp:283-361),
//               plane fit (:702-767), FeatureLine / FeaturePlanVec::ComputeError (Estimator.h:71-83,118-121),
//               fused behind the kNN in the same lane so the 5 neighbours never leave registers.
//   the aligner's time-offset search, which uses the same grid search, lives in time_offset.hip.
// Compiled with -ffp-contract=off.
#include <math.h>
#include <stdlib.h>

#include <cstring>
#include <string.h>

#include "grid_cell_rule.h"
#include "mml_internal.h"
#include "voxel_sort_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// grid build
struct GridDev {
    float ox, oy, oz, inv_cell, cell;
    int dx, dy, dz, ncell;
};

// cell_coord and the exact 5-NN ring search (Knn5, knn5_search, scan_rings01, ...), shared with time_offset.hip
#include "knn5_dev.h"

// A segment of the grid build is one cloud with its own grid.  The segments' points lie behind one offset table; a workgroup serves
// one segment (blockIdx.y), so its table row is wave-uniform and is read through scalar loads.
struct GridSegDev {
    const float4* orig;        // the unsorted cloud
    float4* pts;               // the grid's sorted points
    int* cell_start;
    const uint16_t* tag_orig;  // the points' tags in the order of `orig`; null: the cloud has none
    uint16_t* tags;            // the grid's tags, in the order of `pts`
    GridDev g;
    int off, m;  // the segment's rows in the key / value arrays
};

// Key: unsigned = the cell (one segment), unsigned long long = segment << 32 | cell
template <class Key>
__global__ __launch_bounds__(256) void k_grid_keys(const GridSegDev* __restrict__ tab, Key* __restrict__ keys, unsigned* __restrict__ vals) {
    const GridSegDev& S = tab[blockIdx.y];
    const GridDev g = S.g;
    const int m = S.m, off = S.off;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) {
        const float4 p = S.orig[i];
        const int cx = cell_coord(p.x, g.ox, g.inv_cell, g.dx);
        const int cy = cell_coord(p.y, g.oy, g.inv_cell, g.dy);
        const int cz = cell_coord(p.z, g.oz, g.inv_cell, g.dz);
        const unsigned cell = (unsigned)(cx + g.dx * (cy + g.dy * cz));
        if (sizeof(Key) == 8)
            keys[off + i] = (Key)(((unsigned long long)blockIdx.y << 32) | cell);
        else
            keys[off + i] = (Key)cell;
        vals[off + i] = (unsigned)i;
    }
}

// occupied cells of every segment = key changes inside its rows
template <class Key>
__global__ __launch_bounds__(256) void k_grid_occupied(const GridSegDev* __restrict__ tab, const Key* __restrict__ keys, int* __restrict__ occ) {
    const int m = tab[blockIdx.y].m;
    const Key* k = keys + tab[blockIdx.y].off;
    for (int base = blockIdx.x * 256; base < m; base += gridDim.x * 256) {  // (whole wavefronts: the ballot)
        const int i = base + threadIdx.x;
        const bool head = i < m && (i == 0 || k[i] != k[i - 1]);
        const unsigned long long b = __ballot(head);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd(occ + blockIdx.y, __popcll(b));
    }
}

// the sorted points with their source index in w, and their tags where the cloud has them
__global__ __launch_bounds__(256) void k_grid_gather(const GridSegDev* __restrict__ tab, const unsigned* __restrict__ vals) {
    const GridSegDev& S = tab[blockIdx.y];
    const int m = S.m;
    const unsigned* v = vals + S.off;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) {
        const unsigned src = v[i];
        float4 p = S.orig[src];
        p.w = __uint_as_float(src);
        S.pts[i] = p;
        if (S.tag_orig) S.tags[i] = S.tag_orig[src];
    }
}

// cell_start[c] = first sorted point of the segment whose cell >= c (lower bound); cell_start[ncell] = m.  m = 0: two zero ints.
template <class Key>
__global__ __launch_bounds__(256) void k_grid_cell_start(const GridSegDev* __restrict__ tab, const Key* __restrict__ keys) {
    const GridSegDev& S = tab[blockIdx.y];
    const int m = S.m, ncell = S.g.ncell;
    const Key* k = keys + S.off;
    for (int c = blockIdx.x * 256 + threadIdx.x; c <= ncell; c += gridDim.x * 256) {
        int lo = 0, hi = m;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((unsigned)k[mid] < (unsigned)c)
                lo = mid + 1;
            else
                hi = mid;
        }
        S.cell_start[c] = lo;
    }
}

__global__ __launch_bounds__(256) void k_knn5(MmlGrid g, const float* q, int nq, float max_d2, int* idx, float* d2) {
    int i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < nq;
    Knn5 k;
    knn5_search(g, valid, valid ? q[3 * i] : 0.f, valid ? q[3 * i + 1] : 0.f, valid ? q[3 * i + 2] : 0.f, max_d2, k);
    if (!valid) return;
    for (int j = 0; j < 5; ++j) {
        bool ok = knn_d(k, j) < max_d2 && knn_d(k, 4) < max_d2;
        idx[5 * i + j] = ok ? knn_id(k, j) : -1;
        d2[5 * i + j] = ok ? knn_d(k, j) : INFINITY;
    }
}

#include "eig3_dev.h"

// Eigen 3.3.4 ColPivHouseholderQR<Matrix<double,5,3>>::compute + solve(-1): see oracle/linalg.h.  Register-only:
// the three columns are separate 5-vectors and the column pivoting is done with conditional swaps.
struct Col5 {
    double v[5];
};
__device__ __forceinline__ void col_swap(Col5& a, Col5& b, bool doit) {
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const double x = a.v[r], y = b.v[r];
        a.v[r] = doit ? y : x;
        b.v[r] = doit ? x : y;
    }
}
__device__ __forceinline__ void dswap(double& a, double& b, bool doit) {
    const double x = a, y = b;
    a = doit ? y : x;
    b = doit ? x : y;
}
__device__ __forceinline__ void iswap(int& a, int& b, bool doit) {
    const int x = a, y = b;
    a = doit ? y : x;
    b = doit ? x : y;
}
// Householder step K on column `ck` (rows K..4), applied to the `NO` remaining columns; norm downdate for them.
template <int K>
__device__ __forceinline__ void qr_step(Col5& ck, Col5& o1, Col5& o2, double& nu1, double& nd1, double& nu2, double& nd2,
                                        double& tau_out, bool has1, bool has2) {
    const double tol = 2.2250738585072014e-308;
    const double norm_downdate_threshold = 1.4901161193847656e-08;  // sqrt(eps)
    double tailSqNorm = 0;
#pragma unroll
    for (int r = K + 1; r < 5; ++r) tailSqNorm += ck.v[r] * ck.v[r];
    const double c0 = ck.v[K];
    double tau, beta;
    if (tailSqNorm <= tol) {
        tau = 0;
        beta = c0;
#pragma unroll
        for (int r = K + 1; r < 5; ++r) ck.v[r] = 0;
    } else {
        beta = sqrt(c0 * c0 + tailSqNorm);
        if (c0 >= 0.0) beta = -beta;
#pragma unroll
        for (int r = K + 1; r < 5; ++r) ck.v[r] = ck.v[r] / (c0 - beta);
        tau = (beta - c0) / beta;
    }
    tau_out = tau;
    ck.v[K] = beta;
    if (tau != 0.0) {
        if (has1) {
            double tmp = 0;
#pragma unroll
            for (int r = K + 1; r < 5; ++r) tmp += ck.v[r] * o1.v[r];
            tmp += o1.v[K];
            o1.v[K] -= tau * tmp;
#pragma unroll
            for (int r = K + 1; r < 5; ++r) o1.v[r] -= tau * ck.v[r] * tmp;
        }
        if (has2) {
            double tmp = 0;
#pragma unroll
            for (int r = K + 1; r < 5; ++r) tmp += ck.v[r] * o2.v[r];
            tmp += o2.v[K];
            o2.v[K] -= tau * tmp;
#pragma unroll
            for (int r = K + 1; r < 5; ++r) o2.v[r] -= tau * ck.v[r] * tmp;
        }
    }
    auto downdate = [&](Col5& o, double& nu, double& nd) {
        if (nu != 0.0) {
            double temp = fabs(o.v[K]) / nu;
            temp = (1.0 + temp) * (1.0 - temp);
            temp = temp < 0.0 ? 0.0 : temp;
            const double ratio = nu / nd;
            const double temp2 = temp * (ratio * ratio);
            if (temp2 <= norm_downdate_threshold) {
                double s = 0;
#pragma unroll
                for (int r = K + 1; r < 5; ++r) s += o.v[r] * o.v[r];
                nd = sqrt(s);
                nu = nd;
            } else {
                nu *= sqrt(temp);
            }
        }
    };
    if (has1) downdate(o1, nu1, nd1);
    if (has2) downdate(o2, nu2, nd2);
}

// rank_out (optional): nonzero_pivots, the rank Eigen's solve() uses.
__device__ void plane_fit5(const double (*Ain)[3], double* xout, int* rank_out = nullptr) {
    Col5 c0, c1, c2;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        c0.v[r] = Ain[r][0];
        c1.v[r] = Ain[r][1];
        c2.v[r] = Ain[r][2];
    }
    auto colnorm = [](const Col5& c) {
        double s = 0;
#pragma unroll
        for (int r = 0; r < 5; ++r) s += c.v[r] * c.v[r];
        return sqrt(s);
    };
    double nd0 = colnorm(c0), nd1 = colnorm(c1), nd2 = colnorm(c2);
    double nu0 = nd0, nu1 = nd1, nu2 = nd2;
    const double eps = 2.220446049250313e-16;
    double maxn = nu0;
    if (nu1 > maxn) maxn = nu1;
    if (nu2 > maxn) maxn = nu2;
    const double threshold_helper = (maxn * eps) * (maxn * eps) / 5.0;
    int nonzero_pivots = 3;
    int p0 = 0, p1 = 1, p2 = 2;  // perm: position -> original column
    double tau0, tau1, tau2;
    // ---- k = 0: pivot among columns 0,1,2 (first maximum) ----
    {
        int big = 0;
        double bigv = nu0;
        if (nu1 > bigv) { bigv = nu1; big = 1; }
        if (nu2 > bigv) { bigv = nu2; big = 2; }
        if (nonzero_pivots == 3 && bigv * bigv < threshold_helper * 5.0) nonzero_pivots = 0;
        col_swap(c0, c1, big == 1);
        dswap(nu0, nu1, big == 1);
        dswap(nd0, nd1, big == 1);
        iswap(p0, p1, big == 1);
        col_swap(c0, c2, big == 2);
        dswap(nu0, nu2, big == 2);
        dswap(nd0, nd2, big == 2);
        iswap(p0, p2, big == 2);
        qr_step<0>(c0, c1, c2, nu1, nd1, nu2, nd2, tau0, true, true);
    }
    // ---- k = 1: pivot among columns 1,2 ----
    {
        const bool sw = nu2 > nu1;
        const double bigv = sw ? nu2 : nu1;
        if (nonzero_pivots == 3 && bigv * bigv < threshold_helper * 4.0) nonzero_pivots = 1;
        col_swap(c1, c2, sw);
        dswap(nu1, nu2, sw);
        dswap(nd1, nd2, sw);
        iswap(p1, p2, sw);
        double dum_u = 0, dum_d = 1;
        Col5 dummy = c2;
        qr_step<1>(c1, c2, dummy, nu2, nd2, dum_u, dum_d, tau1, true, false);
    }
    // ---- k = 2 ----
    {
        if (nonzero_pivots == 3 && nu2 * nu2 < threshold_helper * 3.0) nonzero_pivots = 2;
        double du1 = 0, dd1 = 1, du2 = 0, dd2 = 1;
        Col5 dmy1 = c2, dmy2 = c2;
        qr_step<2>(c2, dmy1, dmy2, du1, dd1, du2, dd2, tau2, false, false);
    }
    xout[0] = xout[1] = xout[2] = 0;
    if (rank_out) *rank_out = nonzero_pivots;
    if (nonzero_pivots == 0) return;
    double c[5] = {-1, -1, -1, -1, -1};
    // c = Q^T b : apply H_0, H_1, H_2 (only the first nonzero_pivots reflectors)
    auto apply = [&](const Col5& h, double tau, int K) {
        if (tau != 0.0) {
            double tmp = 0;
#pragma unroll
            for (int r = 0; r < 5; ++r)
                if (r > K) tmp += h.v[r] * c[r];
#pragma unroll
            for (int r = 0; r < 5; ++r)
                if (r == K) tmp += c[r];
#pragma unroll
            for (int r = 0; r < 5; ++r)
                if (r == K) c[r] -= tau * tmp;
#pragma unroll
            for (int r = 0; r < 5; ++r)
                if (r > K) c[r] -= tau * h.v[r] * tmp;
        }
    };
    if (nonzero_pivots > 0) apply(c0, tau0, 0);
    if (nonzero_pivots > 1) apply(c1, tau1, 1);
    if (nonzero_pivots > 2) apply(c2, tau2, 2);
    // back substitution on the leading nonzero_pivots block of R (R(i,j) = column j, row i)
    double y0 = 0, y1 = 0, y2 = 0;
    if (nonzero_pivots > 2) y2 = c[2] / c2.v[2];
    if (nonzero_pivots > 1) {
        double sacc = c[1];
        if (nonzero_pivots > 2) sacc -= c2.v[1] * y2;
        y1 = sacc / c1.v[1];
    }
    {
        double sacc = c[0];
        if (nonzero_pivots > 1) sacc -= c1.v[0] * y1;
        if (nonzero_pivots > 2) sacc -= c2.v[0] * y2;
        y0 = sacc / c0.v[0];
    }
    // dst.row(perm[i]) = c.row(i)
    double x0 = 0, x1 = 0, x2 = 0;
    auto put = [&](int dst, double v) {
        x0 = dst == 0 ? v : x0;
        x1 = dst == 1 ? v : x1;
        x2 = dst == 2 ? v : x2;
    };
    put(p0, y0);
    if (nonzero_pivots > 1) put(p1, y1);
    if (nonzero_pivots > 2) put(p2, y2);
    xout[0] = x0;
    xout[1] = x1;
    xout[2] = x2;
}

// original (unsorted) coordinates of a neighbour are needed in index order: the sorted grid carries xyz next
// to the original index, so the search returns positions; keep a second lookup by original index.
struct AssocParams {
    int first, B, MF;
    MmlGrid g[2];
    const float4* map_orig[2];  // unsorted map clouds (index = original index)
    // global cube map (a12): tagged grids, unsorted clouds, per-cube point counts, grid centre
    MmlGrid gg[2];
    const float4* gmap_orig[2];
    const int* cube_cnt[2];
    int have_g[2];
    int cen[3];
    const float4* ft[2];
    const int* ft_n;
    MmlLineFactor* lf;
    MmlPlaneFactor* pf;
    const double* Twl;  // count x 16
    float thres;     // search bound (float)
    double thres_d;  // gate, compared as in the reference: (double)d2[4] < thres_dist
    int map_m[2];
    int count;
    int fresh_all;  // small batches: every feature goes to the 64- / 32-lane search of k_associate_hard from ring 0
    const int* work_off;
    int* hard_count;   // queue of features whose 5-NN search goes beyond ring 1
    int4* hard_list;
    float* hard_knn;   // 10 floats per queued feature: the top-5 (d2, index) found in rings 0-1
};

// The kernels' argument.  A launch without a bound slot takes AssocParams as it is: every slot is matched against P.g / P.map_orig /
// P.map_m, which live in the kernel arguments.  A launch with a bound slot (BANKED, map banks) carries the device-resident
// descriptor tables -- row 2 * e + kind, e = 0 the context's own map, e = 1 + bank: `table` the local maps, `cube_table` the
// global cube maps -- and the bank of every slot of the context; there P.g / P.map_orig / P.map_m and P.gg / P.gmap_orig /
// P.cube_cnt / P.have_g / P.cen are not read.  Entry 0 of cube_table has have_g = 0 (mml_assoc_ready refuses a launch with a bound
// slot while the context's own cube map is set).
template <bool BANKED>
struct AssocArgs;
template <>
struct AssocArgs<false> : AssocParams {};
template <>
struct AssocArgs<true> : AssocParams {
    const MmlMapDesc* table;
    const MmlCubeDesc* cube_table;
    const int* slot_bank;  // B, indexed by the slot itself
};
static_assert(sizeof(AssocArgs<false>) == sizeof(AssocParams), "the unbanked kernels' argument block is AssocParams");

// The local map of kind `kind` that slot b is matched against.  Unbanked: the kernel arguments.  Banked: the slot's row of the
// table; UNIFORM (b and kind are the same in every lane: one block of k_associate / k_associate_fit_all works on one slot and
// kind) brings the row into scalar registers, as the kernel arguments are -- the search re-reads a descriptor that sits in vector
// registers or memory in front of every row --; otherwise (a far-query group) every lane loads the row of its own entry.
template <bool BANKED, bool UNIFORM>
struct SlotMap;
template <bool UNIFORM>
struct SlotMap<false, UNIFORM> {
    const AssocParams& P;
    int kind;
    __device__ __forceinline__ SlotMap(const AssocArgs<false>& P_, int, int kind_) : P(P_), kind(kind_) {}
    __device__ __forceinline__ const MmlGrid& grid(int ukind) const { return P.g[ukind]; }  // (ukind: the kind as a scalar)
    __device__ __forceinline__ int m() const { return P.map_m[kind]; }
    __device__ __forceinline__ const float4* orig() const { return P.map_orig[kind]; }
};
template <bool UNIFORM>
struct SlotMap<true, UNIFORM> {
    MmlMapDesc d;
    __device__ __forceinline__ SlotMap(const AssocArgs<true>& P, int b, int kind) {
        constexpr int N = sizeof(MmlMapDesc) / 4;
        int w[N];
        if (UNIFORM) {
            const int e = __builtin_amdgcn_readfirstlane(P.slot_bank[b]) + 1;
            const int* src = reinterpret_cast<const int*>(P.table + (2 * e + __builtin_amdgcn_readfirstlane(kind)));
#pragma unroll
            for (int j = 0; j < N; ++j) w[j] = __builtin_amdgcn_readfirstlane(src[j]);
        } else {
            const int* src = reinterpret_cast<const int*>(P.table + (2 * (P.slot_bank[b] + 1) + kind));
#pragma unroll
            for (int j = 0; j < N; ++j) w[j] = src[j];
        }
        __builtin_memcpy(&d, w, sizeof(d));
    }
    __device__ __forceinline__ const MmlGrid& grid(int) const { return d.g; }
    __device__ __forceinline__ int m() const { return d.g.m; }
    __device__ __forceinline__ const float4* orig() const { return d.orig; }
};

// The global cube map of kind `kind` that slot b is matched against first: the cube stage's twin of SlotMap<BANKED, true>, for the
// block-uniform kernels.  Unbanked: the kernel arguments.  Banked: the slot's row of cube_table in scalar registers.
template <bool BANKED>
struct SlotCube;
template <>
struct SlotCube<false> {
    const AssocParams& P;
    int kind;
    __device__ __forceinline__ SlotCube(const AssocArgs<false>& P_, int, int kind_) : P(P_), kind(kind_) {}
    __device__ __forceinline__ const MmlGrid& grid(int ukind) const { return P.gg[ukind]; }
    __device__ __forceinline__ const int* cen() const { return P.cen; }
    __device__ __forceinline__ int have_g() const { return P.have_g[kind]; }
    __device__ __forceinline__ const int* cube_cnt() const { return P.cube_cnt[kind]; }
    __device__ __forceinline__ const float4* orig() const { return P.gmap_orig[kind]; }
};
template <>
struct SlotCube<true> {
    MmlCubeDesc d;
    __device__ __forceinline__ SlotCube(const AssocArgs<true>& P, int b, int kind) {
        constexpr int N = sizeof(MmlCubeDesc) / 4;
        int w[N];
        const int e = __builtin_amdgcn_readfirstlane(P.slot_bank[b]) + 1;
        const int* src = reinterpret_cast<const int*>(P.cube_table + (2 * e + __builtin_amdgcn_readfirstlane(kind)));
#pragma unroll
        for (int j = 0; j < N; ++j) w[j] = __builtin_amdgcn_readfirstlane(src[j]);
        __builtin_memcpy(&d, w, sizeof(d));
    }
    __device__ __forceinline__ const MmlGrid& grid(int) const { return d.g; }
    __device__ __forceinline__ const int* cen() const { return d.cen; }
    __device__ __forceinline__ int have_g() const { return d.have_g; }
    __device__ __forceinline__ const int* cube_cnt() const { return d.cube_cnt; }
    __device__ __forceinline__ const float4* orig() const { return d.orig; }
};
// The far-query kernels' reads, one entry per lane.  The grid a far query searches: the row of its stage (the grid leads both
// row types); the unsorted cloud of its entry's cube map.
__device__ __forceinline__ MmlGrid far_grid(const AssocArgs<true>& P, int b, int kind, int stage) {
    constexpr int N = sizeof(MmlGrid) / 4;
    const int r = 2 * (P.slot_bank[b] + 1) + kind;
    const int* src = stage == 0 ? reinterpret_cast<const int*>(P.cube_table + r) : reinterpret_cast<const int*>(P.table + r);
    int w[N];
#pragma unroll
    for (int j = 0; j < N; ++j) w[j] = src[j];
    MmlGrid g;
    __builtin_memcpy(&g, w, sizeof(g));
    return g;
}
__device__ __forceinline__ const float4* far_cube_orig(const AssocArgs<false>& P, int, int kind) { return P.gmap_orig[kind]; }
__device__ __forceinline__ const float4* far_cube_orig(const AssocArgs<true>& P, int b, int kind) {
    return P.cube_table[2 * (P.slot_bank[b] + 1) + kind].orig;
}

__device__ __forceinline__ void tf_point(const double* T, double x, double y, double z, double& ox, double& oy,
                                         double& oz) {
    ox = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    oy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    oz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

// one lane per feature: grid.x covers MF features, grid.y = slot, grid.z = kind
// model fit + factor record for one feature (a14 / a15 / a16), given its exact 5 nearest map points
__device__ __forceinline__ void store_none(const AssocParams& P, int kind, int b, int i) {
    if (kind == 0) {
        MmlLineFactor out;
        memset(&out, 0, sizeof(out));
        out.src = -1;
        P.lf[(size_t)b * P.MF + i] = out;
    } else {
        MmlPlaneFactor out;
        memset(&out, 0, sizeof(out));
        out.src = -1;
        P.pf[(size_t)b * P.MF + i] = out;
    }
}

// Map_Manager.cpp:583-629 FindUsed{Corner,Surf}Map
__device__ __forceinline__ int find_used_map(float x, float y, float z, const int* cen) {
    int cubeI = int((x + 25.0) / 50.0) + cen[2];
    int cubeJ = int((y + 25.0) / 50.0) + cen[0];
    int cubeK = int((z + 25.0) / 50.0) + cen[1];
    if (x + 25.0 < 0) cubeI--;
    if (y + 25.0 < 0) cubeJ--;
    if (z + 25.0 < 0) cubeK--;
    if (cubeI >= 0 && cubeI < 21 && cubeJ >= 0 && cubeJ < 21 && cubeK >= 0 && cubeK < 11)
        return cubeI + 21 * cubeJ + 21 * 21 * cubeK;  // ToIndex, Map_Manager.cpp:65-67
    return 5000;
}

// The line model of a14 from the 5 neighbours in search order: float centroid and covariance, double eigen-system, the
// gate ev[2] > 3 * ev[1], and the tripod p1 / p2 = centroid +- 0.1 * (eigenvector of ev[2]) stored as floats.  Shared by
// fit_and_store and the test hook mml_model_fit5; p1 / p2 are set only when the model is accepted.
struct LineModel5 {
    float cx, cy, cz;
    double ev[3];
    float p1[3], p2[3];
};
__device__ __forceinline__ bool line_model5(const float* nx, const float* ny, const float* nz, LineModel5& m) {
    float cx = 0, cy = 0, cz = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        cx += nx[j];
        cy += ny[j];
        cz += nz[j];
    }
    cx /= 5;
    cy /= 5;
    cz /= 5;
    float a11 = 0, a12 = 0, a13 = 0, a22 = 0, a23 = 0, a33 = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        float ax = nx[j] - cx, ay = ny[j] - cy, az = nz[j] - cz;
        a11 += ax * ax;
        a12 += ax * ay;
        a13 += ax * az;
        a22 += ay * ay;
        a23 += ay * az;
        a33 += az * az;
    }
    a11 /= 5;
    a12 /= 5;
    a13 /= 5;
    a22 /= 5;
    a23 /= 5;
    a33 /= 5;
    double ud[3];
    eig3_sym(a11, a12, a22, a13, a23, a33, m.ev, ud);
    m.cx = cx;
    m.cy = cy;
    m.cz = cz;
    if (!(m.ev[2] > 3 * m.ev[1])) return false;
    m.p1[0] = cx + 0.1 * ud[0];
    m.p1[1] = cy + 0.1 * ud[1];
    m.p1[2] = cz + 0.1 * ud[2];
    m.p2[0] = cx - 0.1 * ud[0];
    m.p2[1] = cy - 0.1 * ud[1];
    m.p2[2] = cz - 0.1 * ud[2];
    return true;
}

// The plane model of a15 from the 5 neighbours in search order and the selected point s: X of the QR solve, the
// normalised float coefficients, the 0.2 m gate on every neighbour, and the projection of s (set only when accepted).
struct PlaneModel5 {
    double X[3];
    float pa, pb, pc, pd;
    double proj[3];
};
__device__ __forceinline__ bool plane_model5(const float* nx, const float* ny, const float* nz, float sx, float sy, float sz,
                                             PlaneModel5& m) {
    double A[5][3];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        A[j][0] = nx[j];
        A[j][1] = ny[j];
        A[j][2] = nz[j];
    }
    plane_fit5(A, m.X);
    float pa = m.X[0], pb = m.X[1], pc = m.X[2], pd = 1;
    float ps = sqrtf(pa * pa + pb * pb + pc * pc);
    pa /= ps;
    pb /= ps;
    pc /= ps;
    pd /= ps;
    m.pa = pa;
    m.pb = pb;
    m.pc = pc;
    m.pd = pd;
    bool planeValid = true;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        if (fabs((double)(pa * nx[j] + pb * ny[j] + pc * nz[j] + pd)) > 0.2) {
            planeValid = false;
            break;
        }
    }
    if (!planeValid) return false;
    double dist = pa * sx + pb * sy + pc * sz + pd;  // float expression, :740-742
    m.proj[0] = (double)sx - dist * (double)pa;
    m.proj[1] = (double)sy - dist * (double)pb;
    m.proj[2] = (double)sz - dist * (double)pc;
    return true;
}

// returns true (and stores the factor) when the neighbourhood passes the gate and yields a model
__device__ __forceinline__ bool fit_and_store(const AssocParams& P, int kind, int b, int i, const float4 f, const double* T,
                                              float sx, float sy, float sz, bool ok, const Knn5& k, const float4* mp) {
    if (kind == 0) {
        MmlLineFactor out;
        out.src = -1;
        out.error = 0;
        if (ok) {
            float nx[5], ny[5], nz[5];
#pragma unroll
            for (int j = 0; j < 5; j++) {
                float4 q = mp[knn_id(k, j)];
                nx[j] = q.x;
                ny[j] = q.y;
                nz[j] = q.z;
            }
            LineModel5 m;
            if (line_model5(nx, ny, nz, m)) {
                const float x1 = m.p1[0], y1 = m.p1[1], z1 = m.p1[2], x2 = m.p2[0], y2 = m.p2[1], z2 = m.p2[2];
                out.ori[0] = f.x;
                out.ori[1] = f.y;
                out.ori[2] = f.z;
                out.p1[0] = x1;
                out.p1[1] = y1;
                out.p1[2] = z1;
                out.p2[0] = x2;
                out.p2[1] = y2;
                out.p2[2] = z2;
                out.src = i;
                // FeatureLine::ComputeError (Estimator.h:71-83)
                double Px, Py, Pz;
                tf_point(T, f.x, f.y, f.z, Px, Py, Pz);
                double ax = x1, ay = y1, az = z1, bx = x2, by = y2, bz = z2;
                double l12 = sqrt((ax - bx) * (ax - bx) + (ay - by) * (ay - by) + (az - bz) * (az - bz));
                double c0 = (Px - ax) * (Py - by) - (Px - bx) * (Py - ay);
                double c1 = (Px - ax) * (Pz - bz) - (Px - bx) * (Pz - az);
                double c2 = (Py - ay) * (Pz - bz) - (Py - by) * (Pz - az);
                double a012 = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
                out.error = a012 / l12;
            }
        }
        if (out.src >= 0) P.lf[(size_t)b * P.MF + i] = out;
        return out.src >= 0;
    } else {
        MmlPlaneFactor out;
        out.src = -1;
        out.error = 0;
        out._pad = 0;
        if (ok) {
            float nx[5], ny[5], nz[5];
#pragma unroll
            for (int j = 0; j < 5; j++) {
                float4 q = mp[knn_id(k, j)];
                nx[j] = q.x;
                ny[j] = q.y;
                nz[j] = q.z;
            }
            PlaneModel5 m;
            if (plane_model5(nx, ny, nz, sx, sy, sz, m)) {
                out.ori[0] = f.x;
                out.ori[1] = f.y;
                out.ori[2] = f.z;
                out.omega[0] = m.pa;
                out.omega[1] = m.pb;
                out.omega[2] = m.pc;
                out.proj[0] = m.proj[0];
                out.proj[1] = m.proj[1];
                out.proj[2] = m.proj[2];
                double Px, Py, Pz;
                tf_point(T, f.x, f.y, f.z, Px, Py, Pz);
                double ex = Px - out.proj[0], ey = Py - out.proj[1], ez = Pz - out.proj[2];
                out.error = sqrt((ex * ex + ey * ey) + ez * ez);  // Estimator.h:118-121
                out.src = i;
            }
        }
        if (out.src >= 0) P.pf[(size_t)b * P.MF + i] = out;
        return out.src >= 0;
    }
}

// ---- test hook: the model fit above on caller-supplied inputs, one lane per item (mml_model_fit5) ----
__global__ __launch_bounds__(128) void k_model_fit5(int op, const void* in_, long n, void* out_) {
    const long i = (long)blockIdx.x * 128 + threadIdx.x;
    if (i >= n) return;
    if (op == MML_FIT_EIG3) {
        const double* a = (const double*)in_ + 6 * i;
        double* o = (double*)out_ + 12 * i;
        double ev[3], v0[3], v1[3], v2[3];
        eig3_sym(a[0], a[1], a[2], a[3], a[4], a[5], ev, v2, v0, v1);
        for (int r = 0; r < 3; ++r) {
            o[r] = ev[r];
            o[3 + r] = v0[r];
            o[6 + r] = v1[r];
            o[9 + r] = v2[r];
        }
    } else if (op == MML_FIT_QR) {
        const double* a = (const double*)in_ + 15 * i;
        double* o = (double*)out_ + 4 * i;
        double A[5][3], X[3];
        int rank = 0;
        for (int r = 0; r < 5; ++r)
            for (int c = 0; c < 3; ++c) A[r][c] = a[3 * r + c];
        plane_fit5(A, X, &rank);
        o[0] = X[0];
        o[1] = X[1];
        o[2] = X[2];
        o[3] = rank;
    } else if (op == MML_FIT_LINE || op == MML_FIT_PLANE) {
        const int w = op == MML_FIT_LINE ? 15 : 18;
        const float* a = (const float*)in_ + w * i;
        float nx[5], ny[5], nz[5];
        for (int j = 0; j < 5; j++) {
            nx[j] = a[3 * j];
            ny[j] = a[3 * j + 1];
            nz[j] = a[3 * j + 2];
        }
        if (op == MML_FIT_LINE) {
            double* o = (double*)out_ + 13 * i;
            LineModel5 m;
            const bool ok = line_model5(nx, ny, nz, m);
            o[0] = ok ? 1 : 0;
            o[1] = m.cx;
            o[2] = m.cy;
            o[3] = m.cz;
            for (int r = 0; r < 3; ++r) {
                o[4 + r] = m.ev[r];
                o[7 + r] = ok ? m.p1[r] : 0.f;
                o[10 + r] = ok ? m.p2[r] : 0.f;
            }
        } else {
            double* o = (double*)out_ + 11 * i;
            PlaneModel5 m;
            const bool ok = plane_model5(nx, ny, nz, a[15], a[16], a[17], m);
            o[0] = ok ? 1 : 0;
            o[1] = m.X[0];
            o[2] = m.X[1];
            o[3] = m.X[2];
            o[4] = m.pa;
            o[5] = m.pb;
            o[6] = m.pc;
            o[7] = m.pd;
            for (int r = 0; r < 3; ++r) o[8 + r] = ok ? m.proj[r] : 0.0;
        }
    } else if (op == MML_FIT_OPS_F64) {
        const double* a = (const double*)in_ + 2 * i;
        double* o = (double*)out_ + 2 * i;
        o[0] = sqrt(a[0]);
        o[1] = a[0] / a[1];
    } else {
        const float* a = (const float*)in_ + 2 * i;
        float* o = (float*)out_ + 2 * i;
        o[0] = sqrtf(a[0]);
        o[1] = a[0] / a[1];
    }
}

// pass 1: one feature per lane, rings 0 and 1 of the grid privately.  Features whose search is still open are
// queued for pass 2 instead of stalling their wavefront (they cluster spatially, so without the queue a few
// wavefronts full of far queries set the kernel time).
// work decomposition: item = (kind, slot) pair, ceil(nf / 128) workgroup-sized chunks each; work_off is the exclusive
// prefix over the 2 * count items.  A fixed-size grid walks the chunks, so no empty workgroups are dispatched
// (with max_features = 8192 the dense grid spent more time retiring ~30 k empty workgroups than computing).
// (256 threads, four items per thread -- as k_queue_prefix: a sixteen-wavefront workgroup waits for a CU with four free wave slots
//  on every SIMD while another lane's kernel keeps refilling them)
constexpr int AP_THREADS = 256;
__global__ __launch_bounds__(AP_THREADS) void k_assoc_prefix(int first, int count, int B, const int* ft_n, int* work_off, int* hard_count) {
    __shared__ int s_wsum[16];  // totals of the sixteen (slab, wavefront) groups of a 1024-item turn, in item order
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) *hard_count = 0;  // the far-query list of this call starts empty
    const int nitems = 2 * count;
    int acc = 0;  // running prefix over tiles of 1024 items
    for (int t0 = 0; t0 < nitems; t0 += 4 * AP_THREADS) {
        int v[4], x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int it = t0 + q * AP_THREADS + tid;
            v[q] = 0;
            if (it < nitems) {
                const int kind = it / count, slot = it % count;
                const int nf = ft_n[kind * B + first + slot];
                v[q] = nf > 0 ? (nf + 127) / 128 : 0;
            }
        }
        // inclusive scan inside the wavefront (shuffles), then the 16 group totals
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int xx = v[q];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(xx, o);
                if (lane >= o) xx += y;
            }
            x[q] = xx;
            if (lane == 63) s_wsum[q * 4 + wave] = xx;
        }
        __syncthreads();
        int tile = 0, base[4] = {0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int t = s_wsum[w];
            tile += t;
#pragma unroll
            for (int q = 0; q < 4; ++q) base[q] += w < q * 4 + wave ? t : 0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int it = t0 + q * AP_THREADS + tid;
            if (it < nitems) work_off[it] = acc + base[q] + x[q] - v[q];
        }
        acc += tile;
        __syncthreads();
    }
    if (tid == 0) work_off[nitems] = acc;
}

// What pass 1 leaves for a feature, parked in the first 32 bytes of the feature's own (not yet written) factor record:
// [0] = ids 0..3, [1] = (id 4, bits of d2[4], state | stage << 2, cube).
constexpr int REC_NONE = 0, REC_READY = 1, REC_QUEUED = 2;
__device__ __forceinline__ int4* assoc_rec(const AssocParams& P, int kind, int b, int i) {
    return kind == 0 ? reinterpret_cast<int4*>(P.lf + (size_t)b * P.MF + i) : reinterpret_cast<int4*>(P.pf + (size_t)b * P.MF + i);
}
static_assert(sizeof(MmlLineFactor) >= 32 && sizeof(MmlLineFactor) % 16 == 0, "record parking needs 32 aligned bytes");
static_assert(sizeof(MmlPlaneFactor) >= 32 && sizeof(MmlPlaneFactor) % 16 == 0, "record parking needs 32 aligned bytes");

// locate the (kind, slot) item that owns chunk w: last item with work_off[item] <= w
__device__ __forceinline__ int assoc_item(const AssocParams& P, int w) {
    int lo = 0, hi = 2 * P.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P.work_off[mid] <= w)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

constexpr int HARD_REDO = 1 << 30;   // queue entry: search again in the local map (the cube-stage fit failed)
constexpr int HARD_FRESH = 1 << 29;  // queue entry: nothing searched yet, start at ring 0 without a list
// Search only: the model fit (double-precision eigen / QR code, ~150 registers) lives in k_associate_fit_all, so this
// kernel keeps a small register footprint and enough wavefronts in flight to hide its dependent gathers.
// Occupancy the three association kernels are compiled for (wavefronts per SIMD).  The search is a chain of dependent gathers
// (cell offsets, then rows of points): 77 registers gave six wavefronts per SIMD; held to 64 (36 bytes of scratch) it runs
// eight and is 10 % faster (0.289 -> 0.259 ms per 1024 scans); the fit 136 -> 128 registers (three -> four): 0.087 -> 0.080.
// The far-query search loses at 6 (0.073 -> 0.086: 96 bytes of scratch inside its shell loop) and is indifferent at 5.
#ifndef MML_AW_SEARCH
#define MML_AW_SEARCH 8
#define MML_AW_FIT 4
#define MML_AW_HARD 1
#endif
template <bool BANKED>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(MML_AW_SEARCH))) void k_associate(AssocArgs<BANKED> P) {
    const int nitems = 2 * P.count;
    const int total = P.work_off[nitems];
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        const int item = assoc_item(P, w);
        const int kind = item / P.count, slot = item % P.count;
        const int b = slot + P.first;
        const int i = (w - P.work_off[item]) * 128 + threadIdx.x;
        const int nf = P.ft_n[kind * P.B + b];
        const SlotMap<BANKED, true> map(P, b, kind);  // (in front of the first divergent branch: every lane takes part)
        const SlotCube<BANKED> cmap(P, b, kind);
        if (i >= nf) continue;
        int4* rec = assoc_rec(P, kind, b, i);
        const double* T = P.Twl + 16 * slot;
        const float4 f = P.ft[kind][(size_t)b * P.MF + i];
        // Map_Manager.cpp:75-89 pointAssociateToMap: double transform stored to float
        double wx, wy, wz;
        tf_point(T, f.x, f.y, f.z, wx, wy, wz);
        const float sx = wx, sy = wy, sz = wz;
        // :192-196 / :621-625: features outside the 21 x 11 x 21 cube grid, or NaN after the transform, get no factor
        const int cube = find_used_map(sx, sy, sz, cmap.cen());
        // stage 0: the cube's own cloud when it holds > 100 corner / > 50 surf points (:198, :627); stage 1: local map
        const int stage = (cube != 5000 && cmap.have_g() && cmap.cube_cnt()[cube] > (kind == 0 ? 100 : 50)) ? 0 : 1;
        if (cube == 5000 || isnan(sx) || isnan(sy) || isnan(sz) || (stage == 1 && !(map.m() > 20))) {  // (:283 / :702)
            rec[1] = make_int4(0, 0, REC_NONE, 0);
            continue;
        }
        if (P.fresh_all) {
            // A handful of scans cannot fill the device with one lane per feature -- the ~80 candidates of rings 0-1 are then
            // one lane's serial chain (74 us for one scan).  Sixteen lanes per feature share the rows instead.
            const int hw = atomicAdd(P.hard_count, 1);
            P.hard_list[hw] = make_int4(slot, kind, i, stage | (cube << 1) | HARD_FRESH);
            rec[1] = make_int4(0, 0, REC_QUEUED, 0);
            continue;
        }
        // one call site per stage: each names ONE grid of the (wave-uniform) kind, so the grid descriptor stays in scalar
        // registers - selected per lane it is re-read from memory in front of every row
        const int ukind = __builtin_amdgcn_readfirstlane(kind);
        Knn5 k;
        knn_init(k);
        bool done = false;
        int rmax = 0;
        if (stage == 0) {
            const MmlGrid& g = cmap.grid(ukind);
            const KnnQuery q = knn_query(g, sx, sy, sz);
            rmax = (int)ceilf(sqrtf(P.thres) * g.inv_cell) + 1;
            done = scan_rings01(g, q, rmax, P.thres, k, cube);
        } else {
            const MmlGrid& g = map.grid(ukind);
            const KnnQuery q = knn_query(g, sx, sy, sz);
            rmax = (int)ceilf(sqrtf(P.thres) * g.inv_cell) + 1;
            done = scan_rings01(g, q, rmax, P.thres, k, -1);
        }
        if (!done && rmax >= 2) {
            const int hw = atomicAdd(P.hard_count, 1);
            P.hard_list[hw] = make_int4(slot, kind, i, stage | (cube << 1));
            float* hd = P.hard_knn + 10 * (size_t)hw;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                hd[j] = knn_d(k, j);
                hd[5 + j] = __int_as_float(knn_id(k, j));
            }
            rec[1] = make_int4(0, 0, REC_QUEUED, 0);  // finished by k_associate_hard / k_associate_fit
            continue;
        }
        rec[0] = make_int4(knn_id(k, 0), knn_id(k, 1), knn_id(k, 2), knn_id(k, 3));
        rec[1] = make_int4(knn_id(k, 4), __float_as_int(knn_d(k, 4)), REC_READY | (stage << 2), cube);
    }
}

// Model fit of every feature pass 1 finished itself, one lane each.  A feature whose cube neighbourhood (stage 0) yields
// no model is appended to the far-query list with the "search again in the local map" mark (:283 / :702).
template <bool BANKED>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(MML_AW_FIT))) void k_associate_fit_all(AssocArgs<BANKED> P) {
    const int nitems = 2 * P.count;
    const int total = P.work_off[nitems];
    for (int w = blockIdx.x; w < total; w += gridDim.x) {
        const int item = assoc_item(P, w);
        const int kind = item / P.count, slot = item % P.count;
        const int b = slot + P.first;
        const int i = (w - P.work_off[item]) * 128 + threadIdx.x;
        const int nf = P.ft_n[kind * P.B + b];
        const SlotMap<BANKED, true> map(P, b, kind);
        const SlotCube<BANKED> cmap(P, b, kind);
        if (i >= nf) continue;
        const int4* rec = assoc_rec(P, kind, b, i);
        const int4 r0 = rec[0], r1 = rec[1];
        const int state = r1.z & 3, stage = r1.z >> 2, cube = r1.w;
        if (state == REC_QUEUED) continue;
        if (state == REC_NONE) {
            store_none(P, kind, b, i);
            continue;
        }
        const double* T = P.Twl + 16 * slot;
        const float4 f = P.ft[kind][(size_t)b * P.MF + i];
        double wx, wy, wz;
        tf_point(T, f.x, f.y, f.z, wx, wy, wz);
        const float sx = wx, sy = wy, sz = wz;
        Knn5 k;
        knn_init(k);
        const float d5 = __int_as_float(r1.y);  // (the fit reads the five indices and this gate only)
        k.key[0] = knn_key(d5, r0.x);
        k.key[1] = knn_key(d5, r0.y);
        k.key[2] = knn_key(d5, r0.z);
        k.key[3] = knn_key(d5, r0.w);
        k.key[4] = knn_key(d5, r1.x);
        const bool ok = (double)d5 < P.thres_d;  // :201,285 / :631,705
        const bool stored = fit_and_store(P, kind, b, i, f, T, sx, sy, sz, ok, k, stage == 0 ? cmap.orig() : map.orig());
        if (!stored) {
            if (stage == 0 && map.m() > 20) {
                const int hw = atomicAdd(P.hard_count, 1);
                P.hard_list[hw] = make_int4(slot, kind, i, (cube << 1) | HARD_REDO);
            } else {
                store_none(P, kind, b, i);
            }
        }
    }
}

// pass 2: queued features, one 16-lane group each (4 per wavefront).  The group continues from the top-5 list pass 1
// left after ring 1: its lanes split the rows of every further shell and merge their private lists with shuffles
// (xor 8,4,2,1 stays inside the group).  Lane 0 of the group then runs the model fit.
// Queue entry word: bit 0 stage (0 cube cloud, 1 local map), bits 1..14 cube, bit 30 HARD_REDO "search again in the
// local map".

// Far queries, search only: one group of SPAN lanes per queued feature, the lanes split the rows of every shell and merge
// their private top-5 lists with shuffles.  The result goes back to hard_knn; the model fit runs in k_associate_fit with
// one LANE per feature -- inside this kernel it would run on one lane in SPAN.
// round 0: every queued feature, continuing after ring 1 of the stage it was queued in.
// round 1: the features whose cube-stage fit failed (HARD_REDO), local map from ring 0 (:283 / :702).
// SPAN = lanes that share one query (they split the rows of every shell): 4 for batches -- many queries, throughput --, 64 / 32 for
// the live path's handful of scans, where the kernel lasts as long as its slowest query and a far query walks up to 169 rows a shell.
template <int SPAN, bool BANKED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MML_AW_HARD))) void k_associate_hard(AssocArgs<BANKED> P, int round) {
    const int gl = threadIdx.x & (SPAN - 1);
    const int group = (blockIdx.x * 256 + threadIdx.x) / SPAN;
    const int ngroups = (gridDim.x * 256) / SPAN;
    const int total = *P.hard_count;
    for (int w0 = 0; w0 < total; w0 += ngroups) {
        const int w = w0 + group;
        bool live = w < total;
        int slot = 0, kind = 0, i = 0, b = P.first, stage = 1, cube = 0;
        bool fresh = false;
        float sx = 0, sy = 0, sz = 0;
        Knn5 loc, best;
        knn_init(loc);
        knn_init(best);
        if (live) {
            const int4 e = P.hard_list[w];
            if ((round == 1) != ((e.w & HARD_REDO) != 0)) live = false;  // round 0: not the entries k_associate_fit_all appended
            slot = e.x;
            kind = e.y;
            i = e.z;
            stage = round == 1 ? 1 : (e.w & 1);
            cube = (e.w >> 1) & 0x3fff;
            fresh = (e.w & HARD_FRESH) != 0;
            b = slot + P.first;
        }
        if (live) {
            const float4 f = P.ft[kind][(size_t)b * P.MF + i];
            double wx, wy, wz;
            tf_point(P.Twl + 16 * slot, f.x, f.y, f.z, wx, wy, wz);
            sx = wx;
            sy = wy;
            sz = wz;
            if (round == 0 && gl == 0 && !fresh) {  // the list pass 1 left after ring 1
                const float* hd = P.hard_knn + 10 * (size_t)w;
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    loc.key[j] = knn_key(hd[j], __float_as_int(hd[5 + j]));
                }
            }
        }
        const int r0 = (round == 0 && !fresh) ? 2 : 0;
        const float start_d5 = __shfl(knn_d(loc, 4), (threadIdx.x & 63) & ~(SPAN - 1));  // the group's lane 0 (INFINITY unless round 0)
        // the entry's grid descriptor, selected field by field into registers once (a reference to one of four kernel
        // argument structs picked per lane is re-read from memory at every use)
        MmlGrid g = P.g[0];
        if constexpr (BANKED) {
            g = far_grid(P, b, kind, stage);  // the entry's slot and stage name the row (a lane without an entry: the local map of P.first)
        } else {
            const bool k1 = kind == 1, s0 = stage == 0;
            const MmlGrid &a = P.g[1], &c = P.gg[0], &d = P.gg[1];
#define MML_PICK(field) g.field = s0 ? (k1 ? d.field : c.field) : (k1 ? a.field : g.field)
            MML_PICK(pts);
            MML_PICK(cell_start);
            MML_PICK(tags);
            MML_PICK(origin[0]);
            MML_PICK(origin[1]);
            MML_PICK(origin[2]);
            MML_PICK(cell);
            MML_PICK(inv_cell);
            MML_PICK(dim[0]);
            MML_PICK(dim[1]);
            MML_PICK(dim[2]);
#undef MML_PICK
        }
        const int mytag = stage == 0 ? cube : -1;
        const KnnQuery q = knn_query(g, sx, sy, sz);
        const int rmax = live ? (int)ceilf(sqrtf(P.thres) * g.inv_cell) + 1 : 0;
        bool sdone = !live;
        // a query outside the grid: the shells before the grid's near side hold no cell (knn5_search's rnear).  The walk starts at
        // the first shell that does, unless the shell before it already ends the search.
        const int rnear = max(max(max(-q.hx, q.hx - (g.dim[0] - 1)), max(-q.hy, q.hy - (g.dim[1] - 1))), max(-q.hz, q.hz - (g.dim[2] - 1)));
        const int rs = max(r0, rnear);
        if (!sdone && (r0 > rmax || (rs > r0 && (rs > rmax || knn_done(g, q.inset, rs - 1, start_d5, P.thres))))) {
            sdone = true;
            lanes_merge5<SPAN>(loc, best);
        }
        for (int r = rs;; ++r) {
            if (!sdone && r > rmax) sdone = true;
            if (__all(sdone)) break;
            if (!sdone) {
                // the rows of the shell that lie inside the grid, four per lane and turn (scan_shell_rows4)
                const int ylo = max(q.hy - r, 0), yhi = min(q.hy + r, g.dim[1] - 1), zlo = max(q.hz - r, 0), zhi = min(q.hz + r, g.dim[2] - 1);
                const int wy = yhi - ylo + 1, wz = zhi - zlo + 1;
                if (wy > 0 && wz > 0)
                    for (int t = gl; t < wy * wz; t += 4 * SPAN) {
                        // Bound of the group: any upper bound of the final fifth distance (best: merged list of the shells
                        // before this one; loc: this lane's own list; lane 0's starting list of round 0 holds five real points),
                        // and the gate.  P.thres is thres_dist rounded UP to float and a skipped cell holds only points whose
                        // float d2 is above the bound, so no skipped point has (double)d2 < thres_dist.  A list that passes the
                        // gate, (double)d5 < thres_dist, has all five members below P.thres: none of them was skipped, and no
                        // skipped point could have displaced one, so the five ids and d5 are what the unclipped search finds.
                        // Otherwise the true d5 is >= thres_dist, and so is the clipped list's (it is a subset's fifth, or
                        // INFINITY): store_none either way.  Only the list of a query that ends without a factor may differ.
                        const float bound = fminf(fminf(fminf(knn_d(best, 4), knn_d(loc, 4)), start_d5), P.thres);
                        scan_shell_rows4<SPAN>(g, q, r, ylo, wy, zlo, wy * wz, t, loc, mytag, bound);
                    }
            }
            lanes_merge5<SPAN>(loc, best);
            if (!sdone && knn_done(g, q.inset, r, knn_d(best, 4), P.thres)) sdone = true;
        }
        if (live && gl == 0) {
            float* hd = P.hard_knn + 10 * (size_t)w;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                hd[j] = knn_d(best, j);
                hd[5 + j] = __int_as_float(knn_id(best, j));
            }
        }
    }
}

// model fit of the far queries, one lane per queued feature (see k_associate_hard)
template <bool BANKED>
__global__ __launch_bounds__(128) void k_associate_fit(AssocArgs<BANKED> P, int round) {
    const int total = *P.hard_count;
    for (int w = blockIdx.x * 128 + threadIdx.x; w < total; w += gridDim.x * 128) {
        const int4 e = P.hard_list[w];
        if ((round == 1) != ((e.w & HARD_REDO) != 0)) continue;
        const int slot = e.x, kind = e.y, i = e.z, b = slot + P.first;
        const int stage = round == 1 ? 1 : (e.w & 1);
        const float4 f = P.ft[kind][(size_t)b * P.MF + i];
        double wx, wy, wz;
        tf_point(P.Twl + 16 * slot, f.x, f.y, f.z, wx, wy, wz);
        const float sx = wx, sy = wy, sz = wz;
        Knn5 best;
        const float* hd = P.hard_knn + 10 * (size_t)w;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            best.key[j] = knn_key(hd[j], __float_as_int(hd[5 + j]));
        }
        const SlotMap<BANKED, false> map(P, b, kind);
        const bool ok = (double)knn_d(best, 4) < P.thres_d;
        const bool stored = fit_and_store(P, kind, b, i, f, P.Twl + 16 * slot, sx, sy, sz, ok, best,
                                          stage == 0 ? far_cube_orig(P, b, kind) : map.orig());
        if (!stored) {
            if (stage == 0 && map.m() > 20)
                P.hard_list[w].w = e.w | HARD_REDO;  // fall back to the local map (:283 / :702)
            else
                store_none(P, kind, b, i);
        }
        if (round == 1) P.hard_list[w].w = e.w & ~HARD_REDO;
    }
}

// per-slot statistics: counts, used counts, normal Gram matrix (checkLocalizability input)
__global__ __launch_bounds__(256) void k_assoc_stats(int first, int B, int MF, const int* ft_n, const MmlLineFactor* lf,
                                                    const MmlPlaneFactor* pf, double* stats) {
    __shared__ double s_red[4][13];
    const int b = blockIdx.x + first;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[13];
    for (int k = 0; k < 13; ++k) acc[k] = 0;
    const int nl = ft_n[b], np = ft_n[B + b];
    for (int i = tid; i < nl; i += 256) {
        const MmlLineFactor& f = lf[(size_t)b * MF + i];
        if (f.src >= 0) {
            acc[0] += 1;
            if (fabs(f.error) > 1e-5) acc[2] += 1;
        }
    }
    for (int i = tid; i < np; i += 256) {
        const MmlPlaneFactor& f = pf[(size_t)b * MF + i];
        if (f.src >= 0) {
            acc[1] += 1;
            if (fabs(f.error) > 1e-5) acc[3] += 1;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) acc[4 + 3 * r + c] += (double)f.omega[r] * (double)f.omega[c];
        }
    }
    for (int k = 0; k < 13; ++k) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (tid < 13) stats[16 * b + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
}

}  // namespace

extern "C" int mml_model_fit5(mml_ctx* ctx, int op, const void* in, long n, void* out) {
    static const size_t in_bytes[6] = {6 * sizeof(double), 15 * sizeof(double), 15 * sizeof(float),
                                       18 * sizeof(float), 2 * sizeof(double),  2 * sizeof(float)};
    static const size_t out_bytes[6] = {12 * sizeof(double), 4 * sizeof(double), 13 * sizeof(double),
                                        11 * sizeof(double), 2 * sizeof(double), 2 * sizeof(float)};
    if (!ctx || !in || !out || n < 0 || op < 0 || op > MML_FIT_OPS_F32 || n > (long)1 << 26) return MML_ERR_INVALID;
    if (n == 0) return MML_OK;
    int rc = mml_sync_all(ctx);
    if (rc != MML_OK) return rc;
    MmlTemp<char> t_in, t_out;
    bool ok = t_in.alloc(in_bytes[op] * (size_t)n) == hipSuccess && t_out.alloc(out_bytes[op] * (size_t)n) == hipSuccess;
    void *d_in = t_in.d, *d_out = t_out.d;
    ok = ok && hipMemcpy(d_in, in, in_bytes[op] * (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_model_fit5, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, MML_STREAM(ctx), op, (const void*)d_in, n, d_out);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(MML_STREAM(ctx)) == hipSuccess;
    }
    ok = ok && hipMemcpy(out, d_out, out_bytes[op] * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? MML_OK : MML_ERR_HIP;
}

// ---- the grid build: nseg clouds at once ------------------------------------------------------------------------------------------
// A round keys every point by its cell in its segment's own grid and ONE stable radix sort orders all of them.  With several
// segments the key is segment << 32 | cell: the segment is the high word and the rows were in segment order, so a segment's points
// stay in its own rows [off, off + m).  A single cloud (Key = unsigned) is keyed by the cell alone and sorted over exactly the
// bits its cell count needs.
size_t mml_grid_table_bytes(int nseg) { return (sizeof(GridSegDev) + sizeof(int)) * (size_t)nseg; }

// The grids of nseg clouds that are on the device (jobs[g].orig, jobs[g].m points, bounding box jobs[g].bbox_keys): the host takes
// every segment through the rounds of grid_cell_rule.h, one sort, one count and ONE read-back of the nseg counts per round for all
// of them.  A segment that has finished keeps its cell edge and is keyed again in the later rounds of the others: the same keys
// through the same stable sort are the same order, and no second set of buffers has to hold a finished segment's rows.  An empty
// cloud's grid: dim 1 x 1 x 1, cell 1, two zero ints in cell_start.  *rounds: the rounds run = the host synchronisations made.
template <class Key>
int mml_build_grids(mml_ctx* ctx, int nseg, const MmlGridJob* jobs, const MmlGridScratch<Key>& W, int* rounds) {
    static_assert(sizeof(Key) == 4 || sizeof(Key) == 8, "the cell alone, or segment << 32 | cell");
    hipStream_t s = MML_STREAM(ctx);
    MmlStageScope t(ctx, "map_build");
    MML_REQUIRE(sizeof(Key) == 8 || nseg == 1, MML_ERR_INVALID, "grid build: 32-bit keys hold one cloud");
    const size_t tab_bytes = sizeof(GridSegDev) * (size_t)nseg;
    GridSegDev* h_tab = static_cast<GridSegDev*>(W.tab_h);
    const GridSegDev* d_tab = static_cast<const GridSegDev*>(W.tab_d);
    int* occ_h = reinterpret_cast<int*>(static_cast<char*>(W.tab_h) + tab_bytes);
    int* occ_d = reinterpret_cast<int*>(static_cast<char*>(W.tab_d) + tab_bytes);
    const long long max_cells = mml_grid_max_cells(ctx->MM);
    std::vector<float> cell((size_t)nseg);
    std::vector<char> live((size_t)nseg);
    std::vector<float> bbox(6 * (size_t)nseg);
    long long total = 0;
    int max_m = 0;
    for (int g = 0; g < nseg; ++g) {
        const MmlGridJob& J = jobs[g];
        MmlGrid& G = *J.g;
        G.m = J.m;
        cell[g] = J.cell;
        live[g] = J.m > 0;
        for (int c = 0; c < 6; ++c) bbox[6 * (size_t)g + c] = mml_funkey(J.bbox_keys[c]);
        if (J.m == 0) {  // (the empty grid; k_grid_cell_start writes its two zero ints)
            G.dim[0] = G.dim[1] = G.dim[2] = 1;
            G.ncell = 1;
            G.cell = 1.f;
            G.inv_cell = 1.f;
            G.origin[0] = G.origin[1] = G.origin[2] = 0.f;
        }
        memset(static_cast<void*>(&h_tab[g]), 0, sizeof(GridSegDev));
        h_tab[g].orig = J.orig;
        h_tab[g].pts = G.pts;
        h_tab[g].cell_start = G.cell_start;
        h_tab[g].tag_orig = J.tag_orig;
        h_tab[g].tags = G.tags;
        h_tab[g].off = (int)total;
        h_tab[g].m = J.m;
        total += J.m;
        if (J.m > max_m) max_m = J.m;
    }
    MML_REQUIRE(total <= (long long)W.cap, MML_ERR_CAPACITY, "grid build: more points than the scratch holds");
    int seg_bits = 1;
    while ((1 << seg_bits) < nseg) ++seg_bits;
    const int blocks = max_m ? ((max_m + 255) / 256 < 256 ? (max_m + 255) / 256 : 256) : 1;
    *rounds = 0;
    int max_ncell = 1;
    for (int round = 0; total > 0; ++round) {
        for (int g = 0; g < nseg; ++g) {
            MmlGrid& G = *jobs[g].g;
            if (live[g]) {
                int dim[3];
                mml_grid_fit_cell(&bbox[6 * (size_t)g], max_cells, cell[g], dim);
                G.cell = cell[g];
                G.inv_cell = 1.0f / cell[g];
                for (int c = 0; c < 3; ++c) {
                    G.origin[c] = bbox[6 * (size_t)g + c];
                    G.dim[c] = dim[c];
                }
                G.ncell = dim[0] * dim[1] * dim[2];
            }
            h_tab[g].g = GridDev{G.origin[0], G.origin[1], G.origin[2], G.inv_cell, G.cell, G.dim[0], G.dim[1], G.dim[2], G.ncell};
            occ_h[g] = 0;
        }
        MML_HIP(hipMemcpyAsync(W.tab_d, W.tab_h, mml_grid_table_bytes(nseg), hipMemcpyHostToDevice, s));  // (the rows and the zeroed counts)
        hipLaunchKernelGGL(k_grid_keys<Key>, dim3(blocks, nseg), dim3(256), 0, s, d_tab, W.keys, W.vals);
        int end_bit = 32 + seg_bits;
        if (sizeof(Key) == 4)  // (one cloud: the bits of its cell count)
            for (end_bit = 1; (1ll << end_bit) < jobs[0].g->ncell;) ++end_bit;
        const int rt = mml_sort_pairs(ctx, ctx->sort_tmp, W.keys, W.keys2, W.vals, W.vals2, (size_t)total, end_bit, s);
        if (rt != MML_OK) return rt;
        hipLaunchKernelGGL(k_grid_occupied<Key>, dim3(blocks, nseg), dim3(256), 0, s, d_tab, W.keys2, occ_d);
        MML_HIP(hipMemcpyAsync(occ_h, occ_d, sizeof(int) * (size_t)nseg, hipMemcpyDeviceToHost, s));
        MML_HIP(hipStreamSynchronize(s));
        ++*rounds;
        bool again = false;
        for (int g = 0; g < nseg; ++g) {
            if (!live[g]) continue;
            if (mml_grid_refine(jobs[g].m, occ_h[g], round, jobs[g].g->ncell, max_cells)) {
                cell[g] *= 0.5f;
                again = true;
            } else {
                live[g] = 0;
            }
        }
        if (!again) break;
    }
    if (total == 0) {  // (every cloud is empty: the table of the empty grids)
        for (int g = 0; g < nseg; ++g) h_tab[g].g = GridDev{0.f, 0.f, 0.f, 1.f, 1.f, 1, 1, 1, 1};
        MML_HIP(hipMemcpyAsync(W.tab_d, W.tab_h, tab_bytes, hipMemcpyHostToDevice, s));
    }
    for (int g = 0; g < nseg; ++g)
        if (jobs[g].g->ncell > max_ncell) max_ncell = jobs[g].g->ncell;
    if (total > 0) hipLaunchKernelGGL(k_grid_gather, dim3(blocks, nseg), dim3(256), 0, s, d_tab, W.vals2);
    const int cblocks = (max_ncell + 1 + 255) / 256 < 1024 ? (max_ncell + 1 + 255) / 256 : 1024;
    hipLaunchKernelGGL(k_grid_cell_start<Key>, dim3(cblocks, nseg), dim3(256), 0, s, d_tab, W.keys2);
    MML_HIP(hipGetLastError());
    if (total == 0) MML_HIP(hipStreamSynchronize(s));  // (no round has waited for the copy out of the pinned table, which the next build rewrites)
    return MML_OK;
}
template int mml_build_grids<unsigned>(mml_ctx*, int, const MmlGridJob*, const MmlGridScratch<unsigned>&, int*);
template int mml_build_grids<unsigned long long>(mml_ctx*, int, const MmlGridJob*, const MmlGridScratch<unsigned long long>&, int*);

// One cloud of m points into the grid `g`, the unsorted cloud kept in `orig` (filled from h_xyz; null: it is there already): the
// bounding box with its one read-back, then the build with the cell as the whole key, in the context's map_keys / map_vals.
static int build_grid_into(mml_ctx* ctx, MmlGrid& g, float4* orig, const float* h_xyz, int m, float cell,
                           const uint16_t* d_tag_orig) {
    hipStream_t s = MML_STREAM(ctx);
    const int init[6] = MML_BBOX_EMPTY;
    int bbox_keys[6] = MML_BBOX_EMPTY;
    if (m && h_xyz) {  // host xyz (3 floats) -> device float4 (original order, w unused)
        std::vector<float4> tmp((size_t)m);
        for (int i = 0; i < m; ++i) tmp[i] = make_float4(h_xyz[3 * i], h_xyz[3 * i + 1], h_xyz[3 * i + 2], 0.f);
        MML_HIP(hipMemcpyAsync(orig, tmp.data(), sizeof(float4) * (size_t)m, hipMemcpyHostToDevice, s));
        MML_HIP(hipStreamSynchronize(s));  // tmp goes out of scope
    }
    if (m) {
        MmlStageScope t(ctx, "map_build");
        int* d_bbox = ctx->d_misc;
        MML_HIP(hipMemcpyAsync(d_bbox, init, sizeof(init), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_bbox, dim3(256), dim3(256), 0, s, orig, m, d_bbox);
        MML_HIP(hipMemcpyAsync(bbox_keys, d_bbox, sizeof(bbox_keys), hipMemcpyDeviceToHost, s));
        MML_HIP(hipStreamSynchronize(s));
    }
    const int rc = ctx->grid_tab.reserve(ctx, mml_grid_table_bytes(1));
    if (rc != MML_OK) return rc;
    const MmlGridJob job{&g, orig, cell, m, bbox_keys, d_tag_orig};
    const MmlGridScratch<unsigned> W{ctx->map_keys, ctx->map_keys2, ctx->map_vals, ctx->map_vals2, (size_t)ctx->MM, ctx->grid_tab.d, ctx->grid_tab.h};
    int rounds = 0;
    return mml_build_grids(ctx, 1, &job, W, &rounds);
}

int mml_build_grid(mml_ctx* ctx, MmlMapState& map, int kind, const float* h_xyz, int m) {
    MML_REQUIRE(kind == 0 || kind == 1, MML_ERR_INVALID, "map kind must be 0 (corner) or 1 (surf)");
    MML_REQUIRE(m >= 0 && m <= ctx->MM, MML_ERR_CAPACITY, "map larger than max_map_points");
    map.have_map[kind] = false;
    map.grid[kind].tags = nullptr;
    ctx->banks.dirty = true;  // (the descriptor table of a context with banks holds a copy of this grid)
    int rc = build_grid_into(ctx, map.grid[kind], map.map_tmp + (size_t)kind * ctx->MM, h_xyz, m,
                             kind == 0 ? ctx->cfg.cell_corner : ctx->cfg.cell_surf, nullptr);
    if (rc == MML_OK) map.have_map[kind] = true;
    return rc;
}

// a12: the global map handed to Estimate() (Estimator.cpp:1170-1184) as one concatenated cloud with the cube index
// (ToIndex) of every point.  The per-cube kd-trees become one grid whose points carry their cube as a tag.
int mml_cube_match_ensure(mml_ctx* ctx, MmlCubeMatch& G, int kind, int m) {
    MmlGrid& g = G.ggrid[kind];
    if (mml_cube_match_fits(G, kind, m)) return MML_OK;
    const size_t cap = (size_t)(m > 1024 ? m : 1024);
    G.gmap_cap[kind] = 0;
    const int rc = G.ggrid_mem[kind].reserve(
        ctx, {mml_part(g.pts, cap), mml_part(g.cell_start, 4 * (size_t)ctx->MM + 4096 + 2), mml_part(g.tags, cap),
              mml_part(G.gmap_orig[kind], cap), mml_part(G.gtag_orig[kind], cap), mml_part(G.cube_cnt[kind], 4851)});
    if (rc == MML_OK) G.gmap_cap[kind] = (int)cap;
    return rc;
}

int mml_build_global_grid(mml_ctx* ctx, MmlMapState& map, int kind, const float* h_xyz, const int* h_cube, int m, const int* cen) {
    MmlCubeMatch& G = map.cmatch;
    hipStream_t s = MML_STREAM(ctx);
    G.have_gmap[kind] = false;
    ctx->banks.dirty = true;  // (the cube table of a context with banks holds a copy of this map's row)
    if (cen) {
        G.cen[0] = cen[0];
        G.cen[1] = cen[1];
        G.cen[2] = cen[2];
    }
    if (!mml_cube_match_fits(G, kind, m)) MML_HIP(hipStreamSynchronize(s));  // (a copy that grows is replaced with nothing in flight)
    int rc = mml_cube_match_ensure(ctx, G, kind, m);
    if (rc != MML_OK) return rc;
    std::vector<uint16_t> tags((size_t)(m ? m : 1));
    std::vector<int> cnt(4851, 0);
    for (int i = 0; i < m; ++i) {
        tags[i] = (uint16_t)h_cube[i];
        cnt[h_cube[i]]++;
    }
    MML_HIP(hipMemcpyAsync(G.cube_cnt[kind], cnt.data(), sizeof(int) * 4851, hipMemcpyHostToDevice, s));
    if (m) MML_HIP(hipMemcpyAsync(G.gtag_orig[kind], tags.data(), sizeof(uint16_t) * (size_t)m, hipMemcpyHostToDevice, s));
    MML_HIP(hipStreamSynchronize(s));
    rc = build_grid_into(ctx, G.ggrid[kind], G.gmap_orig[kind], h_xyz, m,
                         kind == 0 ? ctx->cfg.cell_corner : ctx->cfg.cell_surf, G.gtag_orig[kind]);
    if (rc == MML_OK) G.have_gmap[kind] = m > 0;
    return rc;
}

int mml_launch_knn5(mml_ctx* ctx, int kind, const float* d_q, int nq, float max_d2, int* d_idx, float* d_d2) {
    MmlStageScope t(ctx, "knn5");
    hipLaunchKernelGGL(k_knn5, dim3((nq + 255) / 256), dim3(256), 0, MML_STREAM(ctx), ctx->own.grid[kind], d_q, nq, max_d2,
                       d_idx, d_d2);
    MML_HIP(hipGetLastError());
    return MML_OK;
}

// the association chain of one launch form: BANKED when a slot of the launch is bound to a map bank
// second_round: some slot of the launch has a cube map to fall back from (the context's own; banked: that of a bound bank)
template <bool BANKED>
static int launch_associate(mml_ctx* ctx, AssocArgs<BANKED>& P, int first, int count, const double* d_Twl, double thres_dist, bool second_round) {
    P.first = first;
    P.B = ctx->B;
    P.MF = ctx->MF;
    const MmlMapState& own = ctx->own;
    for (int k = 0; k < 2; ++k) {
        P.g[k] = own.grid[k];
        P.map_orig[k] = own.map_tmp + (size_t)k * ctx->MM;
        P.ft[k] = ctx->ft_xyz[k];
        P.map_m[k] = own.grid[k].m;
    }
    for (int k = 0; k < 2; ++k) {
        P.gg[k] = own.cmatch.ggrid[k];
        P.gmap_orig[k] = own.cmatch.gmap_orig[k];
        P.cube_cnt[k] = own.cmatch.cube_cnt[k];
        P.have_g[k] = own.cmatch.have_gmap[k] ? 1 : 0;
    }
    P.cen[0] = own.cmatch.cen[0];
    P.cen[1] = own.cmatch.cen[1];
    P.cen[2] = own.cmatch.cen[2];
    P.ft_n = ctx->ft_n;
    P.lf = ctx->lf;
    P.pf = ctx->pf;
    P.Twl = d_Twl;
    P.thres = (float)thres_dist;
    if ((double)P.thres < thres_dist) P.thres = nextafterf(P.thres, INFINITY);
    P.thres_d = thres_dist;
    // queue storage is sliced by slot index (2 * MF entries per slot), the counter by lane
    P.hard_count = ctx->d_misc + 32 + ctx->cur;
    // (a top-level call starts on lane 0 -- mml_step's pieces follow in lane order --, so lane 0 opens a new count)
    ctx->far_lanes = ctx->cur == 0 ? 1 : std::max(ctx->far_lanes, ctx->cur + 1);
    P.hard_list = ctx->hard_list + (size_t)first * ctx->MF * 2;
    P.hard_knn = ctx->hard_knn + (size_t)first * ctx->MF * 2 * 10;
    P.count = count;
    P.fresh_all = count <= 8 ? 1 : 0;
    int* work_off = ctx->work_off + 2 * (size_t)first + ctx->cur;
    P.work_off = work_off;
    {
        MmlStageScope t(ctx, "associate");
        hipLaunchKernelGGL(k_assoc_prefix, dim3(1), dim3(AP_THREADS), 0, MML_STREAM(ctx), first, count, ctx->B, ctx->ft_n, work_off, P.hard_count);
        hipLaunchKernelGGL(k_associate<BANKED>, dim3(4096), dim3(128), 0, MML_STREAM(ctx), P);
    }
    {
        // (before the far-query fit: that one overwrites the parked records of its features with their factors)
        MmlStageScope t(ctx, "associate_fit");
        hipLaunchKernelGGL(k_associate_fit_all<BANKED>, dim3(4096), dim3(128), 0, MML_STREAM(ctx), P);
    }
    {
        MmlStageScope t(ctx, "associate_far");
        // (a whole / half a wavefront per query while all queries of the call -- every feature of up to 4 / 8 scans -- are resident
        //  at once: 2048 workgroups hold 8192 / 16384 of them)
        // lanes per far query of a batch: FOUR.  A batch has tens of thousands of far queries -- throughput, not the slowest query,
        // is what its kernel lasts -- and the lanes of a group split the (y, z) rows of a shell: 25 rows at ring 2 leave a 16-lane
        // group's second turn half empty.  Per 1024 scans (configs[1] / configs[3]): 64 lanes 0.331, 32: 0.224, 16: 0.164 / 0.118,
        // 8: 0.153, 4: 0.147 / 0.113, 2: 0.142 / 0.153, 1: 0.185 ms.
        auto launch_hard = [&](int round) {
            if (!P.fresh_all)
                hipLaunchKernelGGL((k_associate_hard<4, BANKED>), dim3(1024), dim3(256), 0, MML_STREAM(ctx), P, round);
            else if (count <= 4)
                hipLaunchKernelGGL((k_associate_hard<64, BANKED>), dim3(2048), dim3(256), 0, MML_STREAM(ctx), P, round);
            else
                hipLaunchKernelGGL((k_associate_hard<32, BANKED>), dim3(2048), dim3(256), 0, MML_STREAM(ctx), P, round);
        };
        launch_hard(0);
        hipLaunchKernelGGL(k_associate_fit<BANKED>, dim3(512), dim3(128), 0, MML_STREAM(ctx), P, 0);
        if (second_round) {  // features whose cube neighbourhood did not yield a model
            launch_hard(1);
            hipLaunchKernelGGL(k_associate_fit<BANKED>, dim3(512), dim3(128), 0, MML_STREAM(ctx), P, 1);
        }
    }
    for (int i = 0; i < count; ++i) ctx->stats_stale[first + i] = 1;
    MML_HIP(hipGetLastError());
    return MML_OK;
}

int mml_launch_associate(mml_ctx* ctx, int first, int count, const double* d_Twl, double thres_dist, bool with_stats) {
    int rc;
    if (mml_any_bound(ctx, first, count)) {
        // (the entry points bring the device copies up to date before they enqueue anything: mml_assoc_ready)
        MML_REQUIRE(!ctx->banks.dirty && !ctx->own.cmatch.have_gmap[0] && !ctx->own.cmatch.have_gmap[1], MML_ERR_STATE,
                    "association of a bound slot without mml_assoc_ready");
        bool cube = false;
        for (int i = 0; i < count; ++i) {
            const int bank = ctx->banks.slot_bank[(size_t)first + i];
            if (bank >= 0) cube = cube || ctx->banks.bank[(size_t)bank].cmatch.have_gmap[0] || ctx->banks.bank[(size_t)bank].cmatch.have_gmap[1];
        }
        AssocArgs<true> P;
        P.table = ctx->banks.d_table;
        P.cube_table = ctx->banks.d_cube_table;
        P.slot_bank = ctx->banks.d_slot_bank;
        rc = launch_associate<true>(ctx, P, first, count, d_Twl, thres_dist, cube);
    } else {
        AssocArgs<false> P;
        rc = launch_associate<false>(ctx, P, first, count, d_Twl, thres_dist, ctx->own.cmatch.have_gmap[0] || ctx->own.cmatch.have_gmap[1]);
    }
    if (rc != MML_OK) return rc;
    if (with_stats) return mml_ensure_assoc_stats(ctx, first, count);
    return MML_OK;
}

// n_line / n_plane / used counts / normal Gram matrix of the slots' current factors (checkLocalizability's input, Estimator.cpp:536-565;
// the counts k_linearize copies into its records), on the context's current stream, for the slots of the range whose factors changed
// since they were last computed.  mml_step does not ask for them (0.02 ms per 1024 scans of a kernel whose output it never reads).
int mml_ensure_assoc_stats(mml_ctx* ctx, int first, int count) {
    int lo = -1, hi = -1;
    for (int i = 0; i < count; ++i)
        if (ctx->stats_stale[first + i]) {
            if (lo < 0) lo = first + i;
            hi = first + i;
        }
    if (lo < 0) return MML_OK;
    MmlStageScope t(ctx, "assoc_stats");
    hipLaunchKernelGGL(k_assoc_stats, dim3(hi - lo + 1), dim3(256), 0, MML_STREAM(ctx), lo, ctx->B, ctx->MF, ctx->ft_n, ctx->lf, ctx->pf,
                       ctx->assoc_stats);
    MML_HIP(hipGetLastError());
    for (int b = lo; b <= hi; ++b) ctx->stats_stale[b] = 0;
    return MML_OK;
}
