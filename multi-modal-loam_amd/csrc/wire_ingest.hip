// wire_ingest.hip -- the feature node's way in for a batch of union_cloud messages in wire form:
//   mml_scan_upload_wire_plan    the argument rules alone, on the host (wire_decode.h wire_plan)
//   mml_wire_decode_host         the decode on the host (wire_decode.h wire_decode_host)
//   mml_scan_upload_wire_batch   the same rules, then `count` messages into `count` slots: one copy per sensor of the span its
//                                payloads cover, one table (32 bytes per frame), ONE launch of k_wire_decode_batch, one count copy
// The record layouts are those of wire_decode.h and nothing else; mml_scan_upload_wire / mml_scan_upload_pointcloud2 (capi.hip) and
// their kernels are untouched, and tests/test_gpu_wire_batch.py holds this path equal to them byte for byte.
//
// k_wire_decode_batch, grid (tiles of 256 records, frames, 2 sensors): one record per lane, its fields assembled from single-byte
// global loads (wire_decode.h WireBytes) as in the single-message kernels, which this grid repeats per frame.
// MEASURED, NOT ASSUMED (profiles/wire_batch_probe.txt, DESIGN_8F.md): the form that first parks a tile's byte range in LDS --
// a contiguous range of at most MML_WIRE_STAGED bytes, tile = that / record size rounded down to a multiple of 64, the start
// rounded down to 16 bytes, consecutive lanes on consecutive 16-byte words, the fields then taken from LDS as the two dwords
// around an unaligned field and one v_alignbyte_b32 -- was not faster than the single-message kernels on whole frames, so the
// simpler form ships.  The staged form stays compilable for that measurement (make EXTRA=-DMML_WIRE_STAGED=16384) and gives the
// same bytes; the staged spans start on 16 bytes and are followed by 16 spare ones for its rounded loads.
#include <string.h>

#include <algorithm>

#include "mml_internal.h"
#include "wire_decode.h"

namespace {

constexpr int WB_THREADS = 256;
#ifdef MML_WIRE_STAGED
constexpr int WB_TILE_BYTES = MML_WIRE_STAGED;        // payload bytes of a tile, at most (a multiple of 16, at least 64 x 256)
constexpr int WB_LDS_QUADS = WB_TILE_BYTES / 16 + 2;  // + up to 15 bytes in front, the round-up behind, the dword after an unaligned field
static_assert(WB_TILE_BYTES % 16 == 0 && WB_TILE_BYTES >= 64 * 256 && WB_TILE_BYTES <= 32768, "tile bytes");
inline int wb_tile_points(int record_bytes) { return (WB_TILE_BYTES / record_bytes) & ~63; }  // 16 KB, 12 .. 256 bytes: 1344 .. 64 points
#else
inline int wb_tile_points(int) { return WB_THREADS; }
#endif

struct WireFrame {  // per frame: where its two payloads start in the staging buffer (bytes) and how many records each holds
    long long voff, loff;
    int nv, nl;
    int slot, _pad;
};
static_assert(sizeof(WireFrame) == 32, "the table is 32 bytes per frame");

struct WireLayout {
    int point_step, ox, oy, oz, oi, livox_record_bytes, tile_v, tile_l;
};

#ifdef MML_WIRE_STAGED
// The byte source of a tile parked in LDS: position 0 is the tile's first payload byte, `head` bytes into the array.
struct WireLds {
    const uint32_t* w;
    int head;
    __device__ uint32_t le32(int64_t pos) const {
        const int b = head + (int)pos;
        const uint32_t lo = w[b >> 2];
        if ((b & 3) == 0) return lo;
        return __builtin_amdgcn_alignbyte(w[(b >> 2) + 1], lo, (uint32_t)(b & 3));  // ({hi, lo} >> 8 (b & 3)), the low dword
    }
};
#endif

__global__ __launch_bounds__(WB_THREADS) void k_wire_decode_batch(const uint8_t* __restrict__ stage, const WireFrame* __restrict__ tab, WireLayout L,
                                                                  float4* __restrict__ velo_in, mml_livox_point* __restrict__ livox_in, int NV, int NL) {
    const WireFrame f = tab[blockIdx.y];
    const int tid = threadIdx.x, sensor = blockIdx.z;
    const int n = sensor ? f.nl : f.nv, rec = sensor ? L.livox_record_bytes : L.point_step, tile = sensor ? L.tile_l : L.tile_v;
    const long long t0 = (long long)blockIdx.x * tile;
    if (t0 >= n) return;  // (the whole workgroup: no barrier is skipped by a part of it)
    const int m = min(tile, (int)(n - t0));
    const long long b0 = (sensor ? f.loff : f.voff) + t0 * rec;  // the tile's first byte in the staging buffer
#ifdef MML_WIRE_STAGED
    __shared__ uint4 s_q[WB_LDS_QUADS];
    const int head = (int)(b0 & 15);
    const int nq = (head + m * rec + 15) >> 4;  // <= WB_TILE_BYTES / 16 + 1
    const uint4* src = reinterpret_cast<const uint4*>(stage + (b0 - head));
    constexpr int ROUNDS = (WB_TILE_BYTES / 16 + 1 + WB_THREADS - 1) / WB_THREADS;
    uint4 v[ROUNDS];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k)  // (no branch: a lane past the range's end loads its last word again; all loads in flight together)
        v[k] = src[min(tid + k * WB_THREADS, nq - 1)];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k)
        if (tid + k * WB_THREADS < nq) s_q[tid + k * WB_THREADS] = v[k];
    __syncthreads();
    const WireLds bytes{reinterpret_cast<const uint32_t*>(s_q), head};
    const long long base = 0;
#else
    const WireBytes bytes{stage};
    const long long base = b0;
#endif
    if (sensor == 0) {
        uint4* out = reinterpret_cast<uint4*>(velo_in + (size_t)f.slot * NV + t0);
        for (int r = tid; r < m; r += WB_THREADS) {
            uint32_t w[4];
            wire_velo_record(bytes, base + (long long)r * rec, L.ox, L.oy, L.oz, L.oi, w);
            out[r] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        uint32_t* out = reinterpret_cast<uint32_t*>(livox_in + (size_t)f.slot * NL + t0);
        for (int r = tid; r < m; r += WB_THREADS) {
            uint32_t w[5];
            wire_livox_record(bytes, base + (long long)r * rec, rec, w);
#pragma unroll
            for (int k = 0; k < 5; ++k) out[5 * (size_t)r + k] = w[k];
        }
    }
}

WireCall wire_call(int count, const int64_t* velo_at, const int* n_velo, int point_step, int off_x, int off_y, int off_z, int off_intensity,
                   const int64_t* livox_at, const int* n_livox, int livox_record_bytes) {
    return WireCall{count, velo_at, n_velo, point_step, off_x, off_y, off_z, off_intensity, livox_at, n_livox, livox_record_bytes};
}

}  // namespace

extern "C" {

int mml_scan_upload_wire_plan(int count, const int64_t* velo_at, const int* n_velo, int point_step, int off_x, int off_y, int off_z,
                              int off_intensity, const int64_t* livox_at, const int* n_livox, int livox_record_bytes, int max_velo_points,
                              int max_livox_points, int64_t span[4], int* bad_frame) {
    char msg[192];
    return wire_plan(wire_call(count, velo_at, n_velo, point_step, off_x, off_y, off_z, off_intensity, livox_at, n_livox, livox_record_bytes),
                     max_velo_points, max_livox_points, span, bad_frame, msg, sizeof(msg));
}

int mml_wire_decode_host(int count, const uint8_t* velo_data, const int64_t* velo_at, const int* n_velo, int point_step, int off_x, int off_y,
                         int off_z, int off_intensity, const uint8_t* livox_data, const int64_t* livox_at, const int* n_livox,
                         int livox_record_bytes, float* velo_xyzi, mml_livox_point* livox) {
    const WireCall c = wire_call(count, velo_at, n_velo, point_step, off_x, off_y, off_z, off_intensity, livox_at, n_livox, livox_record_bytes);
    char msg[192];
    int64_t span[4];
    const int rc = wire_plan(c, -1, -1, span, nullptr, msg, sizeof(msg));
    if (rc != MML_OK) return rc;
    if ((span[1] > span[0] && (!velo_data || !velo_xyzi)) || (span[3] > span[2] && (!livox_data || !livox))) return MML_ERR_INVALID;
    wire_decode_host(c, velo_data, livox_data, velo_xyzi, livox);
    return MML_OK;
}

int mml_scan_upload_wire_batch(mml_ctx* ctx, int first_slot, int count, const uint8_t* velo_data, const int64_t* velo_at, const int* n_velo,
                               int point_step, int off_x, int off_y, int off_z, int off_intensity, const uint8_t* livox_data,
                               const int64_t* livox_at, const int* n_livox, int livox_record_bytes) {
    if (!ctx) return MML_ERR_INVALID;
    const char* who = "mml_scan_upload_wire_batch";
    // ---- every check, before anything is enqueued or written ----
    if (first_slot < 0 || count < 1 || (long)first_slot + count > ctx->B)
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: slots %d .. %ld outside the context's %d (count %d)", who, first_slot,
                          (long)first_slot + count - 1, ctx->B, count);
    const WireCall c = wire_call(count, velo_at, n_velo, point_step, off_x, off_y, off_z, off_intensity, livox_at, n_livox, livox_record_bytes);
    char msg[192];
    int64_t span[4];
    int bad = -1;
    int rc = wire_plan(c, ctx->cfg.max_velo_points, ctx->cfg.max_livox_points, span, &bad, msg, sizeof(msg));
    if (rc != MML_OK) return mml_refuse(ctx, rc, "%s: %s", who, msg);
    const size_t vbytes = (size_t)(span[1] - span[0]), lbytes = (size_t)(span[3] - span[2]);
    if ((vbytes && !velo_data) || (lbytes && !livox_data))
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: NULL %s with points announced", who, vbytes && !velo_data ? "velo_data" : "livox_data");
    // ---- the slots: as every entry point that touches a slot range ----
    if (hipSetDevice(ctx->device) != hipSuccess) {
        ctx->err = "hipSetDevice failed";
        return MML_ERR_HIP;
    }
    if (!ctx->uploads.empty()) {
        rc = mml_uploads_wait(ctx, first_slot, count);
        if (rc != MML_OK) return rc;
    }
    hipStream_t s = MML_STREAM(ctx);
    // staging buffer: the table, then each sensor's span on a 16-byte boundary with 16 spare bytes behind it (the kernel's rounded
    // loads of the staged form end there).  It grows to the largest call; a growth waits for the stream, like every user of wire_stage.
    MmlCarve<16> carve;
    const MmlField<WireFrame> f_tab = carve.take<WireFrame>((size_t)count);
    const MmlField<uint8_t> f_velo = carve.take<uint8_t>(vbytes + 16), f_livox = carve.take<uint8_t>(lbytes + 16);
    rc = ctx->wire_stage.reserve(ctx, carve.bytes(), s);
    if (rc != MML_OK) return rc;
    // pinned: the table, then the counts as d_n_in holds them
    double* st = mml_stage_alloc(ctx, (sizeof(WireFrame) / sizeof(double) + 1) * (size_t)count);
    WireFrame* tab = reinterpret_cast<WireFrame*>(st);
    int* cnt = reinterpret_cast<int*>(tab + count);
    int max_tiles = 0;
    const WireLayout L{point_step, off_x, off_y, off_z, off_intensity, livox_record_bytes, wb_tile_points(point_step), wb_tile_points(livox_record_bytes)};
    for (int i = 0; i < count; ++i) {
        WireFrame& f = tab[i];
        f.nv = n_velo[i];
        f.nl = n_livox[i];
        f.voff = f.nv ? (long long)f_velo.off + (velo_at[i] - span[0]) : (long long)f_velo.off;
        f.loff = f.nl ? (long long)f_livox.off + (livox_at[i] - span[2]) : (long long)f_livox.off;
        f.slot = first_slot + i;
        f._pad = 0;
        cnt[2 * i] = f.nv;
        cnt[2 * i + 1] = f.nl;
        max_tiles = std::max(max_tiles, std::max((f.nv + L.tile_v - 1) / L.tile_v, (f.nl + L.tile_l - 1) / L.tile_l));
    }
    // ---- at most two payload copies (the gaps between the payloads travel too), the table, one launch, the counts ----
    if (vbytes) MML_HIP(hipMemcpyAsync(f_velo.in(ctx->wire_stage.d), velo_data + span[0], vbytes, hipMemcpyHostToDevice, s));
    if (lbytes) MML_HIP(hipMemcpyAsync(f_livox.in(ctx->wire_stage.d), livox_data + span[2], lbytes, hipMemcpyHostToDevice, s));
    if (max_tiles) {
        MML_HIP(hipMemcpyAsync(f_tab.in(ctx->wire_stage.d), tab, f_tab.bytes(), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_wire_decode_batch, dim3(max_tiles, count, 2), dim3(WB_THREADS), 0, s,
                           reinterpret_cast<const uint8_t*>(ctx->wire_stage.d), f_tab.in(ctx->wire_stage.d), L, ctx->velo_in, ctx->livox_in, ctx->NV,
                           ctx->NL);
        MML_HIP(hipGetLastError());
    }
    MML_HIP(hipMemcpyAsync(ctx->d_n_in + 2 * (size_t)first_slot, cnt, sizeof(int) * 2 * (size_t)count, hipMemcpyHostToDevice, s));
    for (int i = 0; i < count; ++i) {
        ctx->h_n_in[2 * (first_slot + i)] = n_velo[i];
        ctx->raw_extracted[first_slot + i] = 0;
        ctx->h_n_in[2 * (first_slot + i) + 1] = n_livox[i];
    }
    return MML_OK;
}

}  // extern "C"
