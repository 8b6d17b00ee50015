// voxel_sort_dev.h -- the one definition of the sort-based voxel filter's building blocks (pcl::VoxelGrid of PCL 1.8.1 as the
// library's side calls run it) and of the rocPRIM calls behind every sorted grid:
//   arithmetic   mml_fkey / mml_funkey, MML_BBOX_EMPTY, mml_voxel_grid_overflows, MmlVoxGrid -- host and device, no other header
//                needed: a host program can include this file and check the arithmetic on its own (tests/cpp/vox_grid_check.cpp)
//   device       mml_bbox_block_reduce, k_bbox, k_run_heads, mml_voxel_run_sum
//   host         mml_sort_pairs, mml_exclusive_scan, mml_sort_pairs_bytes -- the only place that names rocPRIM's sort and scan
// The device and host parts need mml_internal.h before this file; MML_VOXEL_ARITH_ONLY leaves them (and rocPRIM) out.
// k_voxel (undistort_voxel.hip) restates MmlVoxGrid inside its register budget; a correction to the arithmetic goes to both.
#ifndef MML_VOXEL_SORT_DEV_H
#define MML_VOXEL_SORT_DEV_H

#include <hip/hip_runtime.h>
#include <math.h>

// Order-preserving integer image of a float: a < b as floats <=> key(a) < key(b) as ints (-0.f below +0.f), so that float
// minima and maxima go through integer atomicMin / atomicMax.  mml_funkey is its inverse, bit for bit.
__host__ __device__ inline int mml_fkey(float v) {
    int iv;
    __builtin_memcpy(&iv, &v, sizeof(iv));
    return iv >= 0 ? iv : (iv ^ 0x7fffffff);
}
__host__ __device__ inline float mml_funkey(int key) {
    const int iv = key >= 0 ? key : (key ^ 0x7fffffff);
    float v;
    __builtin_memcpy(&v, &iv, sizeof(v));
    return v;
}
// the empty bounding box as six keys: min x, y, z = +inf, max x, y, z = key(-inf); `const int e[6] = MML_BBOX_EMPTY;`
#define MML_BBOX_EMPTY \
    { 0x7f800000, 0x7f800000, 0x7f800000, (int)0xff800000 ^ 0x7fffffff, (int)0xff800000 ^ 0x7fffffff, (int)0xff800000 ^ 0x7fffffff }

// pcl::VoxelGrid::applyFilter (PCL 1.8.1 voxel_grid.hpp): a bounding box of more than INT_MAX voxels ("Leaf size is too small for the
// input dataset. Integer indices would overflow.") returns the cloud UNFILTERED.  The device filters then key every point by its
// own ordinal, which is the same thing: every voxel holds one point, in input order.
__host__ __device__ inline bool mml_voxel_grid_overflows(const float* mn, const float* mx, float inv) {
    const long long dx = static_cast<long long>((mx[0] - mn[0]) * inv) + 1, dy = static_cast<long long>((mx[1] - mn[1]) * inv) + 1,
                    dz = static_cast<long long>((mx[2] - mn[2]) * inv) + 1;
    return dx * dy * dz > 2147483647LL;
}

// applyFilter's index arithmetic, held bit-equal to the reference: inverse leaf in float, floor (the double overload, of a float
// product) to min_b / div_b, floor(p * inv) - float(min_b), i + j dx + k dx dy.
struct MmlVoxGrid {
    float inv;  // inverse_leaf_size_
    int min_b[3], div_b[3];
    bool overflows;  // the caller's fall-back, see mml_voxel_grid_overflows; index() does not consult it
    __host__ __device__ static MmlVoxGrid make(const float mn[3], const float mx[3], float leaf) {
        MmlVoxGrid g;
        g.inv = 1.0f / leaf;
        for (int c = 0; c < 3; ++c) {
            g.min_b[c] = static_cast<int>(floor(mn[c] * g.inv));
            const int max_b = static_cast<int>(floor(mx[c] * g.inv));
            g.div_b[c] = max_b - g.min_b[c] + 1;
        }
        g.overflows = mml_voxel_grid_overflows(mn, mx, g.inv);
        return g;
    }
    __host__ __device__ unsigned index(float x, float y, float z) const {
        const int ijk0 = static_cast<int>(floor(x * inv) - static_cast<float>(min_b[0]));
        const int ijk1 = static_cast<int>(floor(y * inv) - static_cast<float>(min_b[1]));
        const int ijk2 = static_cast<int>(floor(z * inv) - static_cast<float>(min_b[2]));
        return (unsigned)(ijk0 + ijk1 * div_b[0] + ijk2 * (div_b[0] * div_b[1]));
    }
};
// the grid of a box that was reduced into six keys
__host__ __device__ inline MmlVoxGrid mml_vox_grid_of_keys(const int* bbox_keys, float leaf) {
    const float mn[3] = {mml_funkey(bbox_keys[0]), mml_funkey(bbox_keys[1]), mml_funkey(bbox_keys[2])};
    const float mx[3] = {mml_funkey(bbox_keys[3]), mml_funkey(bbox_keys[4]), mml_funkey(bbox_keys[5])};
    return MmlVoxGrid::make(mn, mx, leaf);
}

#ifndef MML_VOXEL_ARITH_ONLY

#include <rocprim/rocprim.hpp>

// The tail of every bounding-box kernel, for a 256-thread workgroup all of whose lanes arrive: per-lane minima / maxima (+-inf where
// a lane saw no point) -> wave shuffle -> LDS across the four waves -> lanes 0..5 publish into bbox_keys (six keys that started as
// MML_BBOX_EMPTY).  Holds one __syncthreads(), which also orders what the caller wrote to LDS before the call.
__device__ __forceinline__ void mml_bbox_block_reduce(float mn[3], float mx[3], int* bbox_keys) {
    __shared__ float s[6][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < 3; ++c) {
        for (int o = 32; o > 0; o >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], o));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o));
        }
        if (lane == 0) {
            s[c][wave] = mn[c];
            s[3 + c][wave] = mx[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float v = s[c][0];
        for (int w = 1; w < 4; ++w) v = (c < 3) ? fminf(v, s[c][w]) : fmaxf(v, s[c][w]);
        if (c < 3)
            atomicMin(bbox_keys + c, mml_fkey(v));
        else
            atomicMax(bbox_keys + c, mml_fkey(v));
    }
}

// getMinMax3D of a plain array of m points (static: every translation unit that launches it has its own)
static __global__ __launch_bounds__(256) void k_bbox(const float4* pts, int m, int* bbox_keys) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const float4 p = pts[i];
        mn[0] = fminf(mn[0], p.x);
        mn[1] = fminf(mn[1], p.y);
        mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x);
        mx[1] = fmaxf(mx[1], p.y);
        mx[2] = fmaxf(mx[2], p.z);
    }
    mml_bbox_block_reduce(mn, mx, bbox_keys);
}

// flag[i] = 1 where sorted key i starts a run: it differs from its left neighbour above `shift`.  Keys from `limit` on start none.
template <class Key>
__global__ void k_run_heads(const Key* keys, int n, int shift, Key limit, int* flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (keys[i] < limit && (i == 0 || (keys[i] >> shift) != (keys[i - 1] >> shift))) ? 1 : 0;
}

// One lane per voxel, the accumulator of pcl::VoxelGrid: the run of sorted keys that starts at s, summed as floats in input order
// (x, y, z, w from 0.f); returns the run's length.  The four sums do not depend on each other: a caller may ignore sum.w.
template <class Key>
__device__ __forceinline__ int mml_voxel_run_sum(const float4* pts, const Key* keys, const unsigned* vals, int s, int n, int shift,
                                                 float4& sum) {
    const Key vox = keys[s] >> shift;
    float sx = 0, sy = 0, sz = 0, sw = 0;
    int e = s;
    while (e < n && (keys[e] >> shift) == vox) {
        const float4 p = pts[vals[e]];
        sx += p.x;
        sy += p.y;
        sz += p.z;
        sw += p.w;
        ++e;
    }
    sum = make_float4(sx, sy, sz, sw);
    return e - s;
}

// ---- rocPRIM: size query, room in `tmp`, run ----------------------------------------------------------------------------------
// `tmp` is a grow-only owner (the context's sort_tmp, a lane's seg_tmp, a side call's own staging: the stream is drained before a
// live buffer is replaced) or an MmlTmpSpan, a piece of the caller's block that was sized up front and cannot grow.
struct MmlTmpSpan {
    void* d;
    size_t cap;
};
inline int mml_tmp_room(mml_ctx* ctx, MmlStaging<char, false>& tmp, size_t need, hipStream_t s) { return tmp.reserve(ctx, need, s); }
inline int mml_tmp_room(mml_ctx* ctx, MmlTmpSpan& tmp, size_t need, hipStream_t) {
    return need <= tmp.cap ? MML_OK : mml_refuse(ctx, MML_ERR_HIP, "rocPRIM asks for %zu bytes of scratch, %zu were reserved", need, tmp.cap);
}

// stable sort of (key, value) pairs on the keys' bits [0, end_bit)
template <class K, class Tmp>
int mml_sort_pairs(mml_ctx* ctx, Tmp& tmp, const K* keys, K* keys2, const unsigned* vals, unsigned* vals2, size_t n, int end_bit, hipStream_t s) {
    size_t need = 0;
    MML_HIP(rocprim::radix_sort_pairs(nullptr, need, keys, keys2, vals, vals2, n, 0, end_bit, s));
    const int rc = mml_tmp_room(ctx, tmp, need, s);
    if (rc != MML_OK) return rc;
    MML_HIP(rocprim::radix_sort_pairs(tmp.d, need, keys, keys2, vals, vals2, n, 0, end_bit, s));
    return MML_OK;
}
// the temporary storage such a sort asks for (0 when the query fails: the sort itself then reports it), for a caller that must
// not allocate between its launches
template <class K>
size_t mml_sort_pairs_bytes(size_t n, int end_bit, hipStream_t s) {
    size_t need = 0;
    if (rocprim::radix_sort_pairs(nullptr, need, (const K*)nullptr, (K*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr, n, 0, end_bit, s) != hipSuccess) return 0;
    return need;
}
template <class Tmp>
int mml_exclusive_scan(mml_ctx* ctx, Tmp& tmp, const int* in, int* out, size_t n, hipStream_t s) {
    size_t need = 0;
    MML_HIP(rocprim::exclusive_scan(nullptr, need, in, out, 0, n, rocprim::plus<int>(), s));
    const int rc = mml_tmp_room(ctx, tmp, need, s);
    if (rc != MML_OK) return rc;
    MML_HIP(rocprim::exclusive_scan(tmp.d, need, in, out, 0, n, rocprim::plus<int>(), s));
    return MML_OK;
}

#endif  // MML_VOXEL_ARITH_ONLY
#endif
