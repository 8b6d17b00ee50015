// velo_fov.hip -- mml_velo_fov_select[_batch]: the Velodyne field-of-view selection of velo_cloud_handler
// (unionLidarsAligner.cpp:437-490) for n frames per call.  The arithmetic is velo_fov.h, one set of routines for both sides: a
// NULL context runs the reference's loop on the host, a context runs k_vfov_select, ONE workgroup of 256 lanes per frame with the
// frame index in blockIdx.y (hence MML_FOV_BATCH_MAX).
//   The halfPassed flag is the only sequential part of the loop and resolves in parallel: while it is false a point's adjusted ori
// depends on the point and startOri alone, so h = the smallest i whose first-branch ori satisfies ori - startOri > pi is a
// workgroup minimum; points i <= h take the first branch, points i > h the second.
//   A tile is VFOV_BLOCK = 256 consecutive points, lane l of the workgroup holding point 256 t + l of tile t.  Phases:
//     (a) -atan2f of every point, ONCE; lanes 0 and (n - 1) % 256 publish A(0) and A(n-1), which give startOri / endOri;
//     (b) h: per wave the first set bit of a ballot over the tiles in ascending order, then the minimum of the four waves in LDS;
//     (c) final ori, relTime, the FOV predicate;
//     (d) order-preserving compaction: ballot + mbcnt rank inside the wave, the wave totals through LDS, a running base over
//         the tiles; each kept row is one 16-byte store.
//   Phase (b) has to see the whole frame before phase (c) of any tile.  A frame of up to VFOV_REG_POINTS = 4096 points (16 tiles)
// stays in registers across the phases: x, y, z and the azimuth of 16 points per lane.  A larger frame -- a 28 800-point VLP-16
// sweep is one -- takes the same phases with the azimuths parked in the scratch block (4 bytes per point, written and read back
// by the same lane) and the coordinates read a second time in phase (c); atan2f is still evaluated once per point, and there is
// no size above which a frame is refused other than max_velo_points.
//   The rows of frame i land at the frame's input row (the sum of the n_points before it); after the read-back of the counts
// the host knows every frame's packed position and k_vfov_pack moves the rows there, as x, y, z, relTime and / or x, y, z.
// Scratch (one grow-only set owned by the context, mml_mem.h, released by mml_destroy), per input point of the largest call:
// point_step bytes of records (device + pinned), 4 (azimuth), 16 (rows in place), 16 + 12 (the two packed outputs);
// per frame 48 bytes (device + pinned).  Two launches and at most two host synchronisations per call whatever n is.
//   The two halves are stages of their own (vfov_select_stage, vfov_pack_stage): mml_time_offset_estimate_stream (time_offset.hip)
// runs the first and lets the second pack the rows straight into its search's input on the device.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "mml_internal.h"
#include "velo_fov.h"

#define VFOV_BLOCK 256                                 /* points per tile = lanes per workgroup */
#define VFOV_REG_TILES 16                              /* tiles a lane keeps in registers */
#define VFOV_REG_POINTS (VFOV_BLOCK * VFOV_REG_TILES)  /* frames above this park their azimuths in scratch */
#define VFOV_PACK_BLOCKS 32                            /* workgroups per frame of the packing pass (each strides over the frame's rows) */

namespace {

using namespace mml_vfov;

struct VfovFrame {
    long long in_byte;  // the frame's first record in the staged input
    long long row0;     // its first input row = where its kept rows land in `rows` (and its azimuths in `azi`)
    long long dst;      // its first row in the packed outputs (known after the first read-back)
    int n, _pad;
};

struct VfovLayout {
    int step, ox, oy, oz;
    int aligned;  // records and fields are 4-byte aligned: dword loads, else byte loads
};

__device__ __forceinline__ float vfov_load_f32(const uint8_t* p, bool aligned) {
    if (aligned) return *reinterpret_cast<const float*>(p);
    const unsigned u = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
    return __uint_as_float(u);
}

// LDS of one workgroup
struct VfovShared {
    float a_first, a_last;
    int h[4];
    int cnt[2][4];  // wave totals of a tile, double-buffered: one barrier per tile
};

// phase (b) for one tile: the first lane of the wave whose first-branch ori sets the flag (wave-uniform)
__device__ __forceinline__ void vfov_half_tile(bool valid, float a, float startOri, int first_index_of_wave, int& h_wave) {
    const bool sets = valid && vfov_sets_half(vfov_first_branch(a, startOri), startOri);
    const unsigned long long b = __ballot(sets);
    if (b != 0ull && h_wave == 0x7fffffff) h_wave = first_index_of_wave + (__ffsll((long long)b) - 1);
}

// phases (c) and (d) for one tile; `base` = rows kept in the tiles before it (uniform over the workgroup)
__device__ __forceinline__ void vfov_emit_tile(VfovShared& s, int tile, bool valid, int i, int h, float x, float y, float z, float a, float startOri,
                                               float endOri, float4* __restrict__ out, int& base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float ori = i <= h ? vfov_first_branch(a, startOri) : vfov_second_branch(a, endOri);
    const float rel = vfov_rel_time(ori, startOri, endOri);
    const bool keep = valid && vfov_in_fov(ori);
    const unsigned long long b = __ballot(keep);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    int* cnt = s.cnt[tile & 1];
    if (lane == 0) cnt[wave] = __popcll(b);
    __syncthreads();  // (the buffer of tile - 1 is free again once every lane is past this barrier of tile)
    int before = 0, total = 0;
    for (int w = 0; w < 4; ++w) {
        const int c = cnt[w];
        before += w < wave ? c : 0;
        total += c;
    }
    if (keep) out[base + before + rank] = make_float4(x, y, z, rel);
    base += total;
}

__global__ __launch_bounds__(VFOV_BLOCK) void k_vfov_select(const VfovFrame* __restrict__ tab, const uint8_t* __restrict__ raw, VfovLayout L,
                                                            float* __restrict__ azi_all, float4* __restrict__ rows_all,
                                                            mml_velo_fov_info* __restrict__ info) {
    __shared__ VfovShared s;
    const VfovFrame F = tab[blockIdx.y];
    const int n = F.n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (n <= 0) {  // (the whole workgroup)
        if (tid == 0) info[blockIdx.y] = mml_velo_fov_info{0.f, 0.f, -1, 0};
        return;
    }
    const uint8_t* rec = raw + F.in_byte;
    const bool aligned = L.aligned != 0;
    float4* out = rows_all + F.row0;
    const int tiles = (n + VFOV_BLOCK - 1) / VFOV_BLOCK;
    const int i_last = n - 1;
    int h_wave = 0x7fffffff, base = 0;
    float startOri, endOri;
    int h;

    if (n <= VFOV_REG_POINTS) {
        float px[VFOV_REG_TILES], py[VFOV_REG_TILES], pz[VFOV_REG_TILES], pa[VFOV_REG_TILES];
#pragma unroll
        for (int t = 0; t < VFOV_REG_TILES; ++t) {  // (a)
            const int i = t * VFOV_BLOCK + tid;
            px[t] = py[t] = pz[t] = pa[t] = 0.f;
            if (t < tiles && i < n) {
                const uint8_t* p = rec + (size_t)i * L.step;
                px[t] = vfov_load_f32(p + L.ox, aligned);
                py[t] = vfov_load_f32(p + L.oy, aligned);
                pz[t] = vfov_load_f32(p + L.oz, aligned);
                pa[t] = vfov_azimuth(px[t], py[t]);
                if (i == 0) s.a_first = pa[t];
                if (i == i_last) s.a_last = pa[t];
            }
        }
        __syncthreads();
        vfov_sweep(s.a_first, s.a_last, startOri, endOri);
#pragma unroll
        for (int t = 0; t < VFOV_REG_TILES; ++t)  // (b)
            if (t < tiles) vfov_half_tile(t * VFOV_BLOCK + tid < n, pa[t], startOri, t * VFOV_BLOCK + wave * 64, h_wave);
        if (lane == 0) s.h[wave] = h_wave;
        __syncthreads();
        h = min(min(s.h[0], s.h[1]), min(s.h[2], s.h[3]));
#pragma unroll
        for (int t = 0; t < VFOV_REG_TILES; ++t)  // (c), (d)
            if (t < tiles) {
                const int i = t * VFOV_BLOCK + tid;
                vfov_emit_tile(s, t, i < n, i, h, px[t], py[t], pz[t], pa[t], startOri, endOri, out, base);
            }
    } else {
        float* azi = azi_all + F.row0;
        for (int t = 0; t < tiles; ++t) {  // (a)
            const int i = t * VFOV_BLOCK + tid;
            if (i < n) {
                const uint8_t* p = rec + (size_t)i * L.step;
                const float a = vfov_azimuth(vfov_load_f32(p + L.ox, aligned), vfov_load_f32(p + L.oy, aligned));
                azi[i] = a;  // (read back by this lane only)
                if (i == 0) s.a_first = a;
                if (i == i_last) s.a_last = a;
            }
        }
        __syncthreads();
        vfov_sweep(s.a_first, s.a_last, startOri, endOri);
        for (int t = 0; t < tiles; ++t) {  // (b)
            const int i = t * VFOV_BLOCK + tid;
            vfov_half_tile(i < n, i < n ? azi[i] : 0.f, startOri, t * VFOV_BLOCK + wave * 64, h_wave);
        }
        if (lane == 0) s.h[wave] = h_wave;
        __syncthreads();
        h = min(min(s.h[0], s.h[1]), min(s.h[2], s.h[3]));
        for (int t = 0; t < tiles; ++t) {  // (c), (d)
            const int i = t * VFOV_BLOCK + tid;
            float x = 0.f, y = 0.f, z = 0.f, a = 0.f;
            if (i < n) {
                const uint8_t* p = rec + (size_t)i * L.step;
                x = vfov_load_f32(p + L.ox, aligned);
                y = vfov_load_f32(p + L.oy, aligned);
                z = vfov_load_f32(p + L.oz, aligned);
                a = azi[i];
            }
            vfov_emit_tile(s, t, i < n, i, h, x, y, z, a, startOri, endOri, out, base);
        }
    }
    if (tid == 0) info[blockIdx.y] = mml_velo_fov_info{startOri, endOri, h == 0x7fffffff ? -1 : h, base};
}

// the kept rows of every frame from its input row to its packed position, as x, y, z, relTime and / or x, y, z
__global__ __launch_bounds__(256) void k_vfov_pack(const VfovFrame* __restrict__ tab, const mml_velo_fov_info* __restrict__ info,
                                                   const float4* __restrict__ rows, float4* __restrict__ xyzt, float* __restrict__ xyz) {
    const VfovFrame F = tab[blockIdx.y];
    const int kept = info[blockIdx.y].n_kept;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < kept; i += gridDim.x * 256) {
        const float4 r = rows[F.row0 + i];
        if (xyzt) xyzt[F.dst + i] = r;
        if (xyz) {
            float* o = xyz + 3 * (size_t)(F.dst + i);
            o[0] = r.x;
            o[1] = r.y;
            o[2] = r.z;
        }
    }
}

}  // namespace

// Grow-only scratch of the selection, owned by the context.  The entry point drains the stream before it returns, so reserve()
// never replaces a buffer in use.
struct MmlVfovDev {
    MmlStaging<char> io;          // frame table | info rows
    MmlStaging<uint8_t> in;       // the frames' records, each frame 16-byte aligned
    MmlStaging<char, false> big;  // azimuths | rows in place | packed x,y,z,relTime | packed x,y,z
    // the selection these blocks hold (vfov_select_stage), for the packing pass that follows it
    VfovFrame* h_tab = nullptr;
    VfovFrame* d_tab = nullptr;
    size_t tab_bytes = 0;
    mml_velo_fov_info* d_info = nullptr;
    float4* d_rows = nullptr;
    float4* d_packed4 = nullptr;
    float* d_packed3 = nullptr;
    ~MmlVfovDev() {
        io.release();
        in.release();
        big.release();
    }
};

namespace {

// The argument rules of the FOV calls, in the order the calls state them; `outputs_ok` / `capacity_rows` are the caller's own
// (required output pointers present; < 0: refused where the caller wants rows).  A refusal writes nothing.
int vfov_check(mml_ctx* ctx, const char* who, int n, int n_max, bool outputs_ok, bool want_rows, long capacity_rows, const uint8_t* data,
               const long* byte_offsets, const int* n_points, int step, int ox, int oy, int oz) {
    if (n < 1 || n > n_max) return mml_refuse(ctx, MML_ERR_INVALID, "%s: n = %d is outside 1 .. %d", who, n, n_max);
    if (!(byte_offsets && n_points && outputs_ok)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null argument", who);
    if (step < 12) return mml_refuse(ctx, MML_ERR_INVALID, "%s: point_step = %d is below 12", who, step);
    const int offs[3] = {ox, oy, oz};
    for (int c = 0; c < 3; ++c)
        if (offs[c] < 0 || offs[c] > step - 4 || (offs[c] & 3))
            return mml_refuse(ctx, MML_ERR_INVALID, "%s: the offset %d of field %c is outside [0, point_step - 4] or not 4-byte aligned", who, offs[c],
                              "xyz"[c]);
    if (want_rows && capacity_rows < 0) return mml_refuse(ctx, MML_ERR_INVALID, "%s: capacity_rows = %ld is negative", who, capacity_rows);
    long long total_in = 0;
    for (int i = 0; i < n; ++i) {
        if (n_points[i] < 0 || byte_offsets[i] < 0)
            return mml_refuse(ctx, MML_ERR_INVALID, "%s: frame %d: a negative count or offset (%d points at byte %ld)", who, i, n_points[i],
                              byte_offsets[i]);
        total_in += n_points[i];
    }
    if (total_in > 0 && !data) return mml_refuse(ctx, MML_ERR_INVALID, "%s: data is null", who);
    if (ctx)
        for (int i = 0; i < n; ++i)
            if (n_points[i] > ctx->cfg.max_velo_points)
                return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: frame %d: %d points exceed max_velo_points = %d", who, i, n_points[i],
                                  ctx->cfg.max_velo_points);
    return MML_OK;
}

// The selection of n checked frames on the device: the records go down, k_vfov_select runs, counts and info come back -- ONE host
// synchronisation.  *info: the n rows in the pinned block, valid until the context's next selection.  with_packed: room for the
// two packed outputs of vfov_run behind the rows.
int vfov_select_stage(mml_ctx* ctx, const char* who, int n, const uint8_t* data, const long* byte_offsets, const int* n_points, int step, int ox,
                      int oy, int oz, bool with_packed, const mml_velo_fov_info** info) {
    MML_HIP(hipSetDevice(ctx->device));
    long long total_in = 0;
    for (int i = 0; i < n; ++i) total_in += n_points[i];
    MmlCarve<256> io;
    const auto tab = io.take<VfovFrame>((size_t)n);
    const auto inf = io.take<mml_velo_fov_info>((size_t)n);
    MmlCarve<16> in;  // the frames' records, one field per frame: here for the block's size, below again for the offsets
    for (int i = 0; i < n; ++i) in.take<uint8_t>((size_t)n_points[i] * (size_t)step);
    const size_t in_bytes = in.bytes(), rows_in = (size_t)total_in;
    MmlCarve<256> big;
    const auto azi = big.take<float>(rows_in);
    const auto rows = big.take<float4>(rows_in), packed4 = big.take<float4>(with_packed ? rows_in : 0);
    const auto packed3 = big.take<float>(with_packed ? 3 * rows_in : 0);
    MmlVfovDev* d = mml_side<MmlVfovDev>(ctx, MML_SIDE_VELO_FOV);
    if (d->io.reserve(ctx, io.bytes()) || d->in.reserve(ctx, in_bytes ? in_bytes : 16) || d->big.reserve(ctx, big.bytes() ? big.bytes() : 256)) {
        ctx->err = std::string(who) + ": the scratch block could not be grown: " + ctx->err;
        return MML_ERR_HIP;
    }
    VfovFrame* h_tab = tab.in(d->io.h);
    d->h_tab = h_tab;
    d->d_tab = tab.in(d->io.d);
    d->tab_bytes = tab.bytes();
    d->d_info = inf.in(d->io.d);
    d->d_rows = rows.in(d->big.d);
    d->d_packed4 = with_packed ? packed4.in(d->big.d) : nullptr;
    d->d_packed3 = with_packed ? packed3.in(d->big.d) : nullptr;
    {
        MmlCarve<16> at;
        long long row = 0;
        for (int i = 0; i < n; ++i) {
            const auto rec = at.take<uint8_t>((size_t)n_points[i] * (size_t)step);
            if (rec.n) memcpy(rec.in(d->in.h), data + byte_offsets[i], rec.bytes());
            h_tab[i] = VfovFrame{(long long)rec.off, row, 0, n_points[i], 0};
            row += n_points[i];
        }
    }
    const VfovLayout L{step, ox, oy, oz, (step & 3) == 0 ? 1 : 0};
    hipStream_t s = MML_STREAM(ctx);
    {   // the selection's host synchronisation: counts and info
        MmlStageScope t(ctx, "velo_fov");
        MML_HIP(hipMemcpyAsync(d->d_tab, h_tab, tab.bytes(), hipMemcpyHostToDevice, s));
        if (in_bytes) MML_HIP(hipMemcpyAsync(d->in.d, d->in.h, in_bytes, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_vfov_select, dim3(1, (unsigned)n), dim3(VFOV_BLOCK), 0, s, d->d_tab, d->in.d, L, azi.in(d->big.d), d->d_rows,
                           d->d_info);
        MML_HIP(hipGetLastError());
        MML_HIP(hipMemcpyAsync(inf.in(d->io.h), d->d_info, inf.bytes(), hipMemcpyDeviceToHost, s));
        MML_HIP(hipStreamSynchronize(s));
    }
    *info = inf.in(d->io.h);
    return MML_OK;
}

// The packing pass of the selection the blocks hold, enqueued on the stream: frame i's kept rows go to row dst[i] of d_xyzt
// (x, y, z, relTime) and / or d_xyz (x, y, z), device arrays of the caller's.
int vfov_pack_stage(mml_ctx* ctx, int n, const long long* dst, int max_kept, float4* d_xyzt, float* d_xyz) {
    MmlVfovDev* d = mml_side<MmlVfovDev>(ctx, MML_SIDE_VELO_FOV);
    hipStream_t s = MML_STREAM(ctx);
    for (int i = 0; i < n; ++i) d->h_tab[i].dst = dst[i];
    const unsigned bx = (unsigned)((max_kept + 255) / 256);
    MML_HIP(hipMemcpyAsync(d->d_tab, d->h_tab, d->tab_bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_vfov_pack, dim3(bx < (unsigned)VFOV_PACK_BLOCKS ? bx : (unsigned)VFOV_PACK_BLOCKS, (unsigned)n), dim3(256), 0, s, d->d_tab,
                       d->d_info, d->d_rows, d_xyzt, d_xyz);
    MML_HIP(hipGetLastError());
    return MML_OK;
}

int vfov_run(mml_ctx* ctx, const char* who, int n, const uint8_t* data, const long* byte_offsets, const int* n_points, int step, int ox, int oy,
             int oz, float* xyzt, float* xyz, long capacity_rows, int* n_kept, mml_velo_fov_info* info) {
    // ---- checks: all before any work, a refusal writes nothing ----
    const bool want_rows = xyzt || xyz;
    int rc = vfov_check(ctx, who, n, MML_FOV_BATCH_MAX, n_kept != nullptr, want_rows, capacity_rows, data, byte_offsets, n_points, step, ox, oy, oz);
    if (rc != MML_OK) return rc;

    if (!ctx) {  // the host build of the routine
        std::vector<mml_velo_fov_info> inf((size_t)n);
        std::vector<float> rows;
        long long total = 0;
        for (int i = 0; i < n; ++i) {
            if (want_rows) rows.resize(4 * (size_t)(total + n_points[i]));
            vfov_frame_host(data + byte_offsets[i], n_points[i], step, ox, oy, oz, want_rows ? rows.data() + 4 * (size_t)total : nullptr, &inf[i]);
            total += inf[i].n_kept;
        }
        if (want_rows && total > capacity_rows)
            return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: %lld rows are kept, capacity_rows is %ld", who, total, capacity_rows);
        for (int i = 0; i < n; ++i) n_kept[i] = inf[i].n_kept;
        if (info) memcpy(info, inf.data(), sizeof(mml_velo_fov_info) * (size_t)n);
        if (xyzt && total) memcpy(xyzt, rows.data(), sizeof(float) * 4 * (size_t)total);
        if (xyz)
            for (long long r = 0; r < total; ++r) memcpy(xyz + 3 * r, rows.data() + 4 * r, sizeof(float) * 3);
        return MML_OK;
    }

    // ---- device ----
    const mml_velo_fov_info* h_info = nullptr;  // host synchronisation 1 of 2: counts and info
    rc = vfov_select_stage(ctx, who, n, data, byte_offsets, n_points, step, ox, oy, oz, true, &h_info);
    if (rc != MML_OK) return rc;
    MmlVfovDev* d = mml_side<MmlVfovDev>(ctx, MML_SIDE_VELO_FOV);
    hipStream_t s = MML_STREAM(ctx);
    std::vector<long long> dst((size_t)n);
    long long total = 0;
    int max_kept = 0;
    for (int i = 0; i < n; ++i) {
        dst[(size_t)i] = total;
        total += h_info[i].n_kept;
        max_kept = h_info[i].n_kept > max_kept ? h_info[i].n_kept : max_kept;
    }
    if (want_rows && total > capacity_rows)
        return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: %lld rows are kept, capacity_rows is %ld", who, total, capacity_rows);
    if (want_rows && total > 0) {  // host synchronisation 2 of 2: the rows
        MmlStageScope t(ctx, "velo_fov");
        float4* d_xyzt = xyzt ? d->d_packed4 : nullptr;
        float* d_xyz = xyz ? d->d_packed3 : nullptr;
        rc = vfov_pack_stage(ctx, n, dst.data(), max_kept, d_xyzt, d_xyz);
        if (rc != MML_OK) return rc;
        if (xyzt) MML_HIP(hipMemcpyAsync(xyzt, d_xyzt, sizeof(float4) * (size_t)total, hipMemcpyDeviceToHost, s));
        if (xyz) MML_HIP(hipMemcpyAsync(xyz, d_xyz, sizeof(float) * 3 * (size_t)total, hipMemcpyDeviceToHost, s));
        MML_HIP(hipStreamSynchronize(s));
    }
    for (int i = 0; i < n; ++i) n_kept[i] = h_info[i].n_kept;
    if (info) memcpy(info, h_info, sizeof(mml_velo_fov_info) * (size_t)n);
    return MML_OK;
}

}  // namespace

// for mml_time_offset_estimate_stream (time_offset.hip), which keeps the selection on the device: mml_internal.h
int mml_vfov_check(mml_ctx* ctx, const char* who, int n, int n_max, const uint8_t* data, const long* byte_offsets, const int* n_points, int step,
                   int ox, int oy, int oz) {
    return vfov_check(ctx, who, n, n_max, true, false, 0, data, byte_offsets, n_points, step, ox, oy, oz);
}
int mml_vfov_select_device(mml_ctx* ctx, const char* who, int n, const uint8_t* data, const long* byte_offsets, const int* n_points, int step,
                           int ox, int oy, int oz, const mml_velo_fov_info** info) {
    return vfov_select_stage(ctx, who, n, data, byte_offsets, n_points, step, ox, oy, oz, false, info);
}
int mml_vfov_pack_device(mml_ctx* ctx, int n, const long long* dst, int max_kept, float* d_xyz) {
    return vfov_pack_stage(ctx, n, dst, max_kept, nullptr, d_xyz);
}

extern "C" int mml_velo_fov_select_batch(mml_ctx* ctx, int n, const uint8_t* data, const long* byte_offsets, const int* n_points, int point_step,
                                         int off_x, int off_y, int off_z, float* xyzt, float* xyz, long capacity_rows, int* n_kept,
                                         mml_velo_fov_info* info) {
    return vfov_run(ctx, "mml_velo_fov_select_batch", n, data, byte_offsets, n_points, point_step, off_x, off_y, off_z, xyzt, xyz, capacity_rows,
                    n_kept, info);
}

extern "C" int mml_velo_fov_select(mml_ctx* ctx, const uint8_t* data, int n_points, int point_step, int off_x, int off_y, int off_z, float* xyzt,
                                   float* xyz, int capacity_rows, int* n_kept, mml_velo_fov_info* info) {
    const long at = 0;
    return vfov_run(ctx, "mml_velo_fov_select", 1, data, &at, &n_points, point_step, off_x, off_y, off_z, xyzt, xyz, capacity_rows, n_kept, info);
}
