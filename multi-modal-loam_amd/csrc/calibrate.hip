// calibrate.hip -- the aligner node's start-up calibration on the device: hori_cloud_handler's one-time call of calibratePCLICP
// (mm-loam/src/unionLidarsAligner.cpp:221-270, lidars_extrinsic_cali.h:493-618), which yields the _velo_hori_tf_matrix every other
// piece of the aligner takes as an input.  removeFarPointCloud(50) and pcl::VoxelGrid(0.05) on both clouds, then
// pcl::GeneralizedIterativeClosestPoint with setTransformationEpsilon(0.001), setMaxCorrespondenceDistance(2),
// setMaximumIterations(500) from the identity guess.  (setRANSACIterations(12) is set as well; PCL 1.8.1's GICP never reads it.)
//
// What runs where, everything on the ctx stream:
//   k_cv_init      the cloud's header: an empty bounding box, zero counts
//   k_cv_bbox      removeFarPointCloud's test per point ((x*x + y*y) + z*z > far_th*far_th, float, strict), bounding box and number
//                  of the points that stay (getMinMax3D of the cropped cloud; min / max are order-free)
//   k_cv_keys      PCL 1.8.1 voxel_grid.hpp applyFilter's voxel index (MmlVoxGrid, voxel_sort_dev.h).  A cropped point gets a key
//                  above every index, so that the crop needs no compaction and no count on the host; when the box holds more than
//                  INT32_MAX voxels PCL hands the cloud back unfiltered: every point is keyed by its own place, which is the same
//                  thing -- one point per voxel, in input order
//   mml_sort_pairs stable radix sort of (key, place) pairs on the key's 33 bits: a voxel's points stay in input order, which is the
//                  order mmlo_voxel_downsample (oracle/estimate.cpp) sums them in
//   k_run_heads, mml_exclusive_scan, k_cv_centroid
//                  one lane per voxel: float sums of x, y, z, intensity in that order, divided by the count
// mml_cloud_crop_voxel reads the header and the records back in one copy (one host synchronisation).  mml_aligner_calibrate runs
// the chain for both clouds, reads the two headers back (one synchronisation) and hands the filtered clouds, still on the device,
// to the GICP kernels (gicp.hip: one more synchronisation per ten outer iterations run).
// Scratch per point of the larger call seen: 32 bytes of input and output and 32 bytes of keys, places, flags and ranks on the
// device, 32 bytes pinned, plus rocPRIM's temporary storage.  Compiled with -ffp-contract=off.
#include <math.h>
#include <string.h>

#include "mml_internal.h"
#include "voxel_sort_dev.h"

namespace {

struct CvHdr {
    int bbox[6];  // min x, y, z, max x, y, z of the kept points as order-preserving integer images of the floats
    int n_kept;   // points the crop keeps
    int n_out;    // records of the output
    int unfiltered;
    int _pad[3];
};
constexpr unsigned long long CV_DROPPED = 1ull << 32;  // key bit of a cropped point: behind every voxel index
constexpr int CV_KEY_BITS = 33;

__device__ __forceinline__ bool cv_keep(const float4 p, float far2) { return !((p.x * p.x + p.y * p.y) + p.z * p.z > far2); }

__global__ void k_cv_init(CvHdr* h) {
    const int empty[6] = MML_BBOX_EMPTY;
    if (threadIdx.x < 6) h->bbox[threadIdx.x] = empty[threadIdx.x];
    if (threadIdx.x == 6) {
        h->n_kept = 0;
        h->n_out = 0;
        h->unfiltered = 0;
    }
}

__global__ __launch_bounds__(256) void k_cv_bbox(const float4* __restrict__ in, int n, float far2, CvHdr* h) {
    __shared__ int s_cnt[4];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int cnt = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 p = in[i];
        if (!cv_keep(p, far2)) continue;
        ++cnt;
        mn[0] = fminf(mn[0], p.x);
        mn[1] = fminf(mn[1], p.y);
        mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x);
        mx[1] = fmaxf(mx[1], p.y);
        mx[2] = fmaxf(mx[2], p.z);
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    mml_bbox_block_reduce(mn, mx, h->bbox);  // (its barrier also publishes s_cnt)
    if (threadIdx.x == 6) {
        const int t = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        if (t) atomicAdd(&h->n_kept, t);
    }
}

__global__ __launch_bounds__(256) void k_cv_keys(const float4* __restrict__ in, int n, float far2, float leaf, CvHdr* h,
                                                 unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    vals[i] = (unsigned)i;
    if (!cv_keep(p, far2)) {
        keys[i] = CV_DROPPED | (unsigned)i;
        return;
    }
    const MmlVoxGrid g = mml_vox_grid_of_keys(h->bbox, leaf);
    const unsigned idx = g.index(p.x, p.y, p.z);
    keys[i] = g.overflows ? (unsigned)i : idx;
    // (every kept point computes the same answer; the flag only ever goes from 0 to 1)
    if (g.overflows) h->unfiltered = 1;
}

// one lane per voxel: the accumulator of pcl::VoxelGrid<PointXYZI> (float sums in input order, then / n), all four fields
__global__ void k_cv_centroid(const float4* __restrict__ in, const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                              const int* __restrict__ flag, const int* __restrict__ pos, int n, float4* __restrict__ out, CvHdr* h) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    if (s == n - 1) h->n_out = pos[s] + flag[s];
    if (!flag[s]) return;
    if (h->unfiltered) {  // PCL hands the cloud back: a copy (0.f + x would turn a -0.f into +0.f)
        out[pos[s]] = in[vals[s]];
        return;
    }
    float4 sum;
    const float c = static_cast<float>(mml_voxel_run_sum(in, keys, vals, s, n, 0, sum));
    out[pos[s]] = make_float4(sum.x / c, sum.y / c, sum.z / c, sum.w / c);  // (pos[s] < number of heads <= n, the room `out` has)
}

// block (device + pinned twin): the inputs, the headers, the outputs; a cloud's header and its output are what is read back
struct CvIo {
    MmlCarve<16> c;
    MmlField<float4> in;
    MmlField<CvHdr> hdr;
    MmlField<float4> out;
    size_t bytes;
    CvIo(size_t n_pts, size_t n_clouds) : in(c.take<float4>(n_pts)), hdr(c.take<CvHdr>(n_clouds)), out(c.take<float4>(n_pts)), bytes(c.bytes()) {}
};
// work block (device only), for one cloud at a time
struct CvWork {
    MmlCarve<16> c;
    MmlField<unsigned long long> keys, keys2;
    MmlField<unsigned> vals, vals2;
    MmlField<int> flag, pos;
    size_t bytes;
    explicit CvWork(size_t n)
        : keys(c.take<unsigned long long>(n)), keys2(c.take<unsigned long long>(n)), vals(c.take<unsigned>(n)), vals2(c.take<unsigned>(n)),
          flag(c.take<int>(n)), pos(c.take<int>(n)), bytes(c.bytes()) {}
};

}  // namespace

// Grow-only scratch of the calibration calls, owned by the context.  Both entry points drain the stream before they return, so
// reserve() never replaces a buffer in use; nothing a call leaves in them is read by the next.
struct MmlCalibDev {
    MmlStaging<char> io;
    MmlStaging<char, false> work, tmp;
    ~MmlCalibDev() {
        io.release();
        work.release();
        tmp.release();
    }
};

namespace {

// (tmp is sized for the sort here, before anything is launched, so that the chain is not held up by an allocation; were the scan
//  to ask for more, mml_exclusive_scan would drain the stream and grow it)
int cv_reserve(mml_ctx* ctx, MmlCalibDev* d, const CvIo& io, size_t n_max) {
    const size_t need = mml_sort_pairs_bytes<unsigned long long>(n_max, CV_KEY_BITS, MML_STREAM(ctx));
    const CvWork w(n_max);
    if (d->io.reserve(ctx, io.bytes) || d->work.reserve(ctx, w.bytes) || d->tmp.reserve(ctx, need ? need : 1)) return MML_ERR_HIP;
    return MML_OK;
}

// enqueues crop + voxel filter of the n > 0 device points `in`: header to *hdr, records to out[0 .. hdr->n_out)
int cv_launch(mml_ctx* ctx, MmlCalibDev* d, const float4* in, int n, float far_th, float leaf, CvHdr* hdr, float4* out) {
    hipStream_t s = MML_STREAM(ctx);
    MmlStageScope t(ctx, "crop_voxel");
    const CvWork w((size_t)n);
    char* g = d->work.d;
    const float far2 = far_th * far_th;
    const int blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_cv_init, dim3(1), dim3(64), 0, s, hdr);
    hipLaunchKernelGGL(k_cv_bbox, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, s, in, n, far2, hdr);
    hipLaunchKernelGGL(k_cv_keys, dim3(blocks), dim3(256), 0, s, in, n, far2, leaf, hdr, w.keys.in(g), w.vals.in(g));
    MML_HIP(hipGetLastError());
    int rc = mml_sort_pairs(ctx, d->tmp, w.keys.in(g), w.keys2.in(g), w.vals.in(g), w.vals2.in(g), (size_t)n, CV_KEY_BITS, s);
    if (rc != MML_OK) return rc;
    // (a cropped point starts no run)
    hipLaunchKernelGGL(k_run_heads<unsigned long long>, dim3(blocks), dim3(256), 0, s, w.keys2.in(g), n, 0, CV_DROPPED, w.flag.in(g));
    rc = mml_exclusive_scan(ctx, d->tmp, w.flag.in(g), w.pos.in(g), (size_t)n, s);
    if (rc != MML_OK) return rc;
    hipLaunchKernelGGL(k_cv_centroid, dim3(blocks), dim3(256), 0, s, in, w.keys2.in(g), w.vals2.in(g), w.flag.in(g), w.pos.in(g), n, out, hdr);
    MML_HIP(hipGetLastError());
    return MML_OK;
}

bool cv_positive(float v) { return isfinite(v) && v > 0.f; }

}  // namespace

extern "C" int mml_cloud_crop_voxel(mml_ctx* ctx, const float* xyzi, int n, float far_th, float leaf, float* out_xyzi, int capacity,
                                    int* n_out, int* unfiltered) {
    if (!ctx) return MML_ERR_INVALID;
    if (n < 0 || (n > 0 && !xyzi) || !n_out) return mml_refuse(ctx, MML_ERR_INVALID, "mml_cloud_crop_voxel: a null argument or n = %d < 0", n);
    if (!cv_positive(far_th) || !cv_positive(leaf))
        return mml_refuse(ctx, MML_ERR_INVALID, "mml_cloud_crop_voxel: far_th = %g, leaf = %g must be positive and finite", far_th, leaf);
    if (out_xyzi && capacity < 0) return mml_refuse(ctx, MML_ERR_INVALID, "mml_cloud_crop_voxel: capacity = %d < 0", capacity);
    int rc = mml_enter_idle(ctx);
    if (rc != MML_OK) return rc;
    *n_out = 0;
    if (unfiltered) *unfiltered = 0;
    if (n == 0) return MML_OK;
    const CvIo io((size_t)n, 1);
    MmlCalibDev* d = mml_side<MmlCalibDev>(ctx, MML_SIDE_CALIB);
    rc = cv_reserve(ctx, d, io, (size_t)n);
    if (rc != MML_OK) return rc;
    hipStream_t s = MML_STREAM(ctx);
    char *h = d->io.h, *g = d->io.d;
    memcpy(io.in.in(h), xyzi, io.in.bytes());
    MML_HIP(hipMemcpyAsync(io.in.in(g), io.in.in(h), io.in.bytes(), hipMemcpyHostToDevice, s));
    rc = cv_launch(ctx, d, io.in.in(g), n, far_th, leaf, io.hdr.in(g), io.out.in(g));
    if (rc != MML_OK) return rc;
    // header | records: one copy (the sizing call takes the header alone)
    MML_HIP(hipMemcpyAsync(io.hdr.in(h), io.hdr.in(g), (out_xyzi ? io.out.end() : io.hdr.end()) - io.hdr.off, hipMemcpyDeviceToHost, s));
    MML_HIP(hipStreamSynchronize(s));
    const CvHdr& H = *io.hdr.in(h);
    *n_out = H.n_out;
    if (unfiltered) *unfiltered = H.unfiltered;
    if (!out_xyzi) return MML_OK;
    if (capacity < H.n_out) return mml_refuse(ctx, MML_ERR_CAPACITY, "mml_cloud_crop_voxel: %d records, room for %d", H.n_out, capacity);
    memcpy(out_xyzi, io.out.in(h), sizeof(float4) * (size_t)H.n_out);
    return MML_OK;
}

extern "C" int mml_aligner_calibrate(mml_ctx* ctx, const float* hori_xyzi, int n_hori, const float* velo_xyzi, int n_velo, float* hori_tf,
                                     float* velo_hori_tf, int* converged, mml_calib_info* info) {
    if (!ctx) return MML_ERR_INVALID;
    if (n_hori < 0 || n_velo < 0 || (n_hori > 0 && !hori_xyzi) || (n_velo > 0 && !velo_xyzi) || !hori_tf || !velo_hori_tf || !converged)
        return mml_refuse(ctx, MML_ERR_INVALID, "mml_aligner_calibrate: a null argument or a negative count");
    if ((size_t)n_hori + (size_t)n_velo > 0x7fffffffull)
        return mml_refuse(ctx, MML_ERR_CAPACITY, "mml_aligner_calibrate: %zu points in one call", (size_t)n_hori + (size_t)n_velo);
    int rc = mml_enter_idle(ctx);
    if (rc != MML_OK) return rc;
    *converged = 0;
    mml_calib_info I;
    memset(&I, 0, sizeof(I));
    I.n_hori_in = n_hori;
    I.n_velo_in = n_velo;
    if (info) *info = I;
    constexpr float FAR_TH = 50.f, LEAF = 0.05f;                  // removeFarPointCloud(.., 50), setLeafSize(0.05f, ..)
    const mml_gicp_opts opts = {500, 1e-3, 2.0};                  // setMaximumIterations, setTransformationEpsilon, setMaxCorrespondenceDistance
    const int n[2] = {n_hori, n_velo};
    const float* src[2] = {hori_xyzi, velo_xyzi};
    const size_t first[2] = {0, (size_t)n_hori};
    const CvIo io((size_t)n_hori + (size_t)n_velo, 2);
    MmlCalibDev* d = mml_side<MmlCalibDev>(ctx, MML_SIDE_CALIB);
    const float4 *d_out[2] = {nullptr, nullptr};
    int n_ds[2] = {0, 0}, unf[2] = {0, 0};
    if (n_hori + n_velo > 0) {
        rc = cv_reserve(ctx, d, io, (size_t)(n_hori > n_velo ? n_hori : n_velo));
        if (rc != MML_OK) return rc;
        hipStream_t s = MML_STREAM(ctx);
        char *h = d->io.h, *g = d->io.d;
        for (int k = 0; k < 2; ++k) {
            if (n[k] == 0) continue;
            memcpy(io.in.in(h) + first[k], src[k], sizeof(float4) * (size_t)n[k]);
            MML_HIP(hipMemcpyAsync(io.in.in(g) + first[k], io.in.in(h) + first[k], sizeof(float4) * (size_t)n[k], hipMemcpyHostToDevice, s));
            rc = cv_launch(ctx, d, io.in.in(g) + first[k], n[k], FAR_TH, LEAF, io.hdr.in(g) + k, io.out.in(g) + first[k]);
            if (rc != MML_OK) return rc;
            d_out[k] = io.out.in(g) + first[k];
        }
        MML_HIP(hipMemcpyAsync(io.hdr.in(h), io.hdr.in(g), io.hdr.bytes(), hipMemcpyDeviceToHost, s));
        MML_HIP(hipStreamSynchronize(s));
        for (int k = 0; k < 2; ++k)
            if (n[k] > 0) {
                n_ds[k] = io.hdr.in(h)[k].n_out;
                unf[k] = io.hdr.in(h)[k].unfiltered;
            }
    }
    I.n_hori_ds = n_ds[0];
    I.n_velo_ds = n_ds[1];
    I.hori_unfiltered = unf[0];
    I.velo_unfiltered = unf[1];
    float T[16];
    rc = mml_gicp_align_device(ctx, "mml_aligner_calibrate", d_out[0], n_ds[0], d_out[1], n_ds[1], &opts, T, converged, &I.gicp);
    if (rc != MML_OK) return rc;
    if (info) *info = I;
    if (!*converged) return MML_OK;
    memcpy(hori_tf, T, sizeof(T));
    // _velo_hori_tf_matrix (unionLidarsAligner.cpp:251-253): block(0,0,3,3) = R^T, block(0,3,3,1) = -t, row 3 = hori_tf's row 3.
    // This is the reference's matrix, not the rigid inverse [R^T | -R^T t].
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) velo_hori_tf[4 * r + c] = T[4 * c + r];
        velo_hori_tf[4 * r + 3] = T[4 * r + 3] * -1.f;
    }
    for (int c = 0; c < 4; ++c) velo_hori_tf[12 + c] = T[12 + c];
    return MML_OK;
}
