// livox_stream.hip -- the aligner node's steady-state work (unionLidarsAligner.cpp) on the device:
//   :736-763  transform_hori_timestamp      mml_livox_stream_push*: k_stream_stamp / k_stream_decode
//   :766-868  pub_horipoints_given_stamp    mml_union_assemble: k_union_plan (which points), k_union_gather (the records)
//   :872-1009 the same, one-stamp overload  mml_union_assemble_offset: k_union_plan_offset, k_union_gather
//   :350-352  pcl::transformPointCloud      k_union_gather's Velodyne blocks (the expression of k_tofs_tf, time_offset.hip)
// The stream is a flat array of 20-byte records (5 dwords each) and a flat array of 64-bit stamps; point i (counted over everything
// ever pushed) sits at element i - base.  The frame recurrence itself is union_plan.h, shared with the host's mml_union_plan.
// Compiled with -ffp-contract=off.
#include <string.h>

#include "mml_internal.h"
#include "union_plan.h"

struct mml_livox_stream {
    mml_ctx* ctx = nullptr;
    long cap = 0;
    uint32_t* rec[2] = {nullptr, nullptr};  // two arrays of cap records: the live part moves from one to the other when the end is reached
    uint64_t* stamp[2] = {nullptr, nullptr};
    int cur = 0;
    long base = 0, front = 0, tail = 0;  // absolute point indices: element 0 of the current array, the queue's front, one past its last point
    uint64_t hs = 0;
    bool have_hs = false;
    unsigned long long* d_disorder = nullptr;  // time-order violations counted by the push kernels
    unsigned long long* h_disorder = nullptr;  // pinned
    uint8_t* wire = nullptr;                   // 19 * cap bytes, allocated by the first push_wire
    MmlFixed mem;                              // owns all of the above
};

// What mml_union_assemble keeps on the context: the small tables (pinned twin) and the Velodyne rows on their way in.  Grow-only;
// the call drains the stream before it returns, so reserve() never replaces a buffer in use.
struct MmlUnionDev {
    MmlStaging<char> io;
    MmlStaging<float4, false> velo;
    ~MmlUnionDev() {
        io.release();
        velo.release();
    }
};

namespace {

constexpr int UNION_CHUNK = 1024;       // frames k_union_plan resolves per round out of LDS
constexpr int UNION_GATHER_BLOCKS = 64;  // workgroups per frame and part of k_union_gather (each strides over its part)

// :751-758 for the points of one message that already lie in the record array (struct form): stamp and time-order check.
// A point is compared with the one before it in the stream, by absolute time hs + S as the frame cut compares them.
__global__ __launch_bounds__(256) void k_stream_stamp(const uint32_t* __restrict__ rec, uint64_t* __restrict__ stamp, long pos, int n,
                                                      uint64_t delta, uint64_t hs, int has_prev, unsigned long long* __restrict__ disorder) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint64_t S = delta + rec[5 * (size_t)(pos + j)];
    uint64_t prev = S;
    if (j > 0)
        prev = delta + rec[5 * (size_t)(pos + j - 1)];
    else if (has_prev)
        prev = stamp[pos - 1];
    stamp[pos + j] = S;
    if (hs + S < hs + prev) atomicAdd(disorder, 1ull);
}

__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// The same for a message in wire form (19-byte little-endian records, see mml_scan_upload_wire): decode, stamp, check.
__global__ __launch_bounds__(256) void k_stream_decode(const uint8_t* __restrict__ wire, uint32_t* __restrict__ rec, uint64_t* __restrict__ stamp,
                                                       long pos, int n, uint64_t delta, uint64_t hs, int has_prev,
                                                       unsigned long long* __restrict__ disorder) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint8_t* p = wire + 19 * (size_t)j;
    uint32_t* r = rec + 5 * (size_t)(pos + j);
    const uint32_t off = load_u32_unaligned(p);
    r[0] = off;
    r[1] = load_u32_unaligned(p + 4);
    r[2] = load_u32_unaligned(p + 8);
    r[3] = load_u32_unaligned(p + 12);
    r[4] = (uint32_t)p[16] | ((uint32_t)p[17] << 8) | ((uint32_t)p[18] << 16);
    const uint64_t S = delta + off;
    uint64_t prev = S;
    if (j > 0)
        prev = delta + load_u32_unaligned(p - 19);
    else if (has_prev)
        prev = stamp[pos - 1];
    stamp[pos + j] = S;
    if (hs + S < hs + prev) atomicAdd(disorder, 1ull);
}

// Which points every frame takes.  ONE workgroup; per round of UNION_CHUNK frames:
//   1. every lane: the lower bounds of the round's frame boundaries over the live stamps [q0, tail) (frame i ends where frame
//      i + 1 starts, so a round of c frames needs c + 1 searches); they do not depend on the front;
//   2. lane 0: the front's recurrence over the round, out of LDS (union_plan.h; integers only, no stamp is read);
//   3. every lane: its frames' rows and the slots' counts, each from the front its frame started with.
// A stream with time-order violations is refused: *verdict says so and nothing else is written.
__global__ __launch_bounds__(256) void k_union_plan(const uint64_t* __restrict__ S, long base, long q0, long tail, uint64_t hs, int count,
                                                    const uint64_t* __restrict__ stamps, const int* __restrict__ voff, int first_slot,
                                                    int max_livox_points, const unsigned long long* __restrict__ disorder,
                                                    mml_union_frame* __restrict__ rows, unsigned long long* __restrict__ verdict,
                                                    int* __restrict__ n_in) {
    __shared__ long s_lb[UNION_CHUNK + 1];
    __shared__ long s_q[UNION_CHUNK + 1];
    const unsigned long long bad = *disorder;
    if (threadIdx.x == 0) *verdict = bad;
    if (bad) return;  // (the whole workgroup)
    if (threadIdx.x == 0) s_q[0] = q0;
    for (int c0 = 0; c0 < count; c0 += UNION_CHUNK) {
        const int c = count - c0 < UNION_CHUNK ? count - c0 : UNION_CHUNK;
        for (int t = threadIdx.x; t <= c; t += 256) s_lb[t] = mml_union_lower_bound(S, base, q0, tail, hs, stamps[c0 + t]);
        __syncthreads();
        if (threadIdx.x == 0) {
            long q = s_q[0];
            mml_union_frame f;
            for (int t = 0; t < c; ++t) {
                q = mml_union_resolve(q, tail, s_lb[t], s_lb[t + 1], max_livox_points, &f);
                s_q[t + 1] = q;
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < c; t += 256) {
            mml_union_frame f;
            mml_union_resolve(s_q[t], tail, s_lb[t], s_lb[t + 1], max_livox_points, &f);
            rows[c0 + t] = f;
            n_in[2 * (size_t)(first_slot + c0 + t)] = voff[c0 + t + 1] - voff[c0 + t];
            n_in[2 * (size_t)(first_slot + c0 + t) + 1] = f.status == MML_UNION_OK ? f.n_livox : 0;
        }
        __syncthreads();
        if (threadIdx.x == 0) s_q[0] = s_q[c];
    }
}

// The same for the one-stamp overload (:872-1009, mml_union_assemble_offset): frame i takes up to `sliced` points from the
// first one at or after starts[i].  The three phases of k_union_plan with one search per frame (a round of c frames needs c, not
// c + 1: a frame has no end stamp) and mml_union_resolve_offset as the recurrence.  The recurrence is a clamp-add
// (q' = min(max(q, lb) + sliced, tail)), so a wave scan could replace lane 0's loop; at about 40 cycles per frame that loop is
// shorter than the Velodyne copy the launch waits behind, and the serial form is the one the host runs too.
__global__ __launch_bounds__(256) void k_union_plan_offset(const uint64_t* __restrict__ S, long base, long q0, long tail, uint64_t hs, int count,
                                                           const uint64_t* __restrict__ starts, const int* __restrict__ voff, int first_slot,
                                                           int sliced, const unsigned long long* __restrict__ disorder,
                                                           mml_union_frame* __restrict__ rows, unsigned long long* __restrict__ verdict,
                                                           int* __restrict__ n_in) {
    __shared__ long s_lb[UNION_CHUNK];
    __shared__ long s_q[UNION_CHUNK + 1];
    const unsigned long long bad = *disorder;
    if (threadIdx.x == 0) *verdict = bad;
    if (bad) return;  // (the whole workgroup)
    if (threadIdx.x == 0) s_q[0] = q0;
    for (int c0 = 0; c0 < count; c0 += UNION_CHUNK) {
        const int c = count - c0 < UNION_CHUNK ? count - c0 : UNION_CHUNK;
        for (int t = threadIdx.x; t < c; t += 256) s_lb[t] = mml_union_lower_bound(S, base, q0, tail, hs, starts[c0 + t]);
        __syncthreads();
        if (threadIdx.x == 0) {
            long q = s_q[0];
            mml_union_frame f;
            for (int t = 0; t < c; ++t) {
                q = mml_union_resolve_offset(q, tail, s_lb[t], sliced, &f);
                s_q[t + 1] = q;
            }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < c; t += 256) {
            mml_union_frame f;
            mml_union_resolve_offset(s_q[t], tail, s_lb[t], sliced, &f);
            rows[c0 + t] = f;
            n_in[2 * (size_t)(first_slot + c0 + t)] = voff[c0 + t + 1] - voff[c0 + t];
            n_in[2 * (size_t)(first_slot + c0 + t) + 1] = f.n_livox;  // (0 unless OK)
        }
        __syncthreads();
        if (threadIdx.x == 0) s_q[0] = s_q[c];
    }
}

// The records.  Grid (2 * UNION_GATHER_BLOCKS at most, frame): blocks [0, gl) of a frame copy its Livox points, the others
// transform its Velodyne rows.
//   Livox: the frame's source [begin, end) is contiguous, so it is copied as a stream of dwords, consecutive lanes on consecutive
//   dwords of source and destination (both 4-byte aligned); dword 0 of a record becomes the truncated hs + S[k] - start (:814,
//   :823) and the top byte of dword 4 (_pad, which roscpp leaves unset) becomes 0.
//   Velodyne: pcl::transformPointCloud (PCL 1.8.1 common/impl/transforms.hpp), float, left to right; tf == nullptr: copy.
__global__ __launch_bounds__(256) void k_union_gather(const mml_union_frame* __restrict__ rows, const unsigned long long* __restrict__ verdict,
                                                      const uint32_t* __restrict__ rec, const uint64_t* __restrict__ S, long base, uint64_t hs,
                                                      const uint64_t* __restrict__ stamps, const float4* __restrict__ vin,
                                                      const int* __restrict__ voff, const float* __restrict__ tf, int first_slot, int gl,
                                                      float4* __restrict__ velo_in, int NV, uint32_t* __restrict__ livox_in, int NL) {
    if (*verdict) return;
    const int f = blockIdx.y;
    const size_t slot = (size_t)(first_slot + f);
    if ((int)blockIdx.x < gl) {
        if (rows[f].status != MML_UNION_OK) return;
        const int nd = 5 * rows[f].n_livox;  // (n_livox <= max_livox_points <= NL)
        const long b = rows[f].begin - base;
        const uint32_t* src = rec + 5 * (size_t)b;
        const uint64_t* Sp = S + b;
        const uint64_t shift = hs - stamps[f];
        uint32_t* dst = livox_in + 5 * slot * (size_t)NL;
        for (int d = blockIdx.x * 256 + threadIdx.x; d < nd; d += gl * 256) {
            const int k = d / 5, r = d - 5 * k;
            uint32_t v = src[d];
            if (r == 0)
                v = (uint32_t)(Sp[k] + shift);
            else if (r == 4)
                v &= 0x00ffffffu;
            dst[d] = v;
        }
    } else {
        const int n = voff[f + 1] - voff[f], row0 = voff[f] - voff[0];
        const int gv = (int)gridDim.x - gl;
        float4* dst = velo_in + slot * (size_t)NV;
        for (int i = ((int)blockIdx.x - gl) * 256 + threadIdx.x; i < n; i += gv * 256) {
            const float4 p = vin[row0 + i];
            float4 o = p;
            if (tf) {
                o.x = tf[0] * p.x + tf[1] * p.y + tf[2] * p.z + tf[3];
                o.y = tf[4] * p.x + tf[5] * p.y + tf[6] * p.z + tf[7];
                o.z = tf[8] * p.x + tf[9] * p.y + tf[10] * p.z + tf[11];
            }
            dst[i] = o;
        }
    }
}

// io block: what goes down in one copy (stamps, offsets, tf), then what comes back in one copy (the rows with the verdict
// directly behind them: 32-byte rows, so it is 8-byte aligned)
struct UnionIo {
    MmlCarve<256> c;
    MmlField<uint64_t> stamps;
    MmlField<int> voff;
    MmlField<float> tf;
    MmlField<mml_union_frame> rows;
    MmlField<unsigned long long> verdict;
    size_t down_bytes, up_bytes, bytes;
    explicit UnionIo(size_t count)
        : stamps(c.take<uint64_t>(count + 1)), voff(c.take<int>(count + 1)), tf(c.take<float>(16)), rows(c.take<mml_union_frame>(count)),
          verdict(c.pack<unsigned long long>(1)), down_bytes(rows.off), up_bytes(verdict.end() - rows.off), bytes(c.bytes()) {}
};

// Room for n more points: when the current array's end would be passed, the live part moves to the front of the other array.
// Source and destination are different allocations, so the copies cannot overlap; they are ordered on the stream like everything else.
int stream_make_room(mml_livox_stream* s, int n) {
    mml_ctx* ctx = s->ctx;
    if (s->tail - s->base + n <= s->cap) return MML_OK;
    const long live = s->tail - s->front, at = s->front - s->base;
    if (live > 0) {
        MML_HIP(hipMemcpyAsync(s->rec[1 - s->cur], s->rec[s->cur] + 5 * (size_t)at, 20 * (size_t)live, hipMemcpyDeviceToDevice, MML_STREAM(ctx)));
        MML_HIP(hipMemcpyAsync(s->stamp[1 - s->cur], s->stamp[s->cur] + at, sizeof(uint64_t) * (size_t)live, hipMemcpyDeviceToDevice,
                               MML_STREAM(ctx)));
    }
    s->cur = 1 - s->cur;
    s->base = s->front;
    return MML_OK;
}

int stream_push(mml_livox_stream* s, const char* who, uint64_t timebase, const void* pts, int n, bool wire) {
    if (!s) return MML_ERR_INVALID;
    mml_ctx* ctx = s->ctx;
    if (n < 0 || (n > 0 && !pts)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: %s", who, n < 0 ? "negative point count" : "null point buffer");
    if ((s->tail - s->front) + n > s->cap)
        return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: %ld live points + %d exceed capacity_points = %ld", who, s->tail - s->front, n, s->cap);
    MML_HIP(hipSetDevice(ctx->device));
    if (wire && n > 0 && !s->wire) MML_HIP(s->mem.alloc(&s->wire, 19 * (size_t)s->cap));
    if (!s->have_hs) {  // :203-207, whatever the message holds
        s->hs = timebase;
        s->have_hs = true;
    }
    if (n == 0) return MML_OK;
    int rc = stream_make_room(s, n);
    if (rc != MML_OK) return rc;
    hipStream_t st = MML_STREAM(ctx);
    const long pos = s->tail - s->base;
    const int has_prev = s->tail > s->front ? 1 : 0;
    const uint64_t delta = timebase - s->hs;
    uint32_t* rec = s->rec[s->cur];
    uint64_t* stamp = s->stamp[s->cur];
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (wire) {
        MML_HIP(hipMemcpyAsync(s->wire, pts, 19 * (size_t)n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_stream_decode, dim3(blocks), dim3(256), 0, st, s->wire, rec, stamp, pos, n, delta, s->hs, has_prev, s->d_disorder);
    } else {
        MML_HIP(hipMemcpyAsync(rec + 5 * (size_t)pos, pts, 20 * (size_t)n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_stream_stamp, dim3(blocks), dim3(256), 0, st, rec, stamp, pos, n, delta, s->hs, has_prev, s->d_disorder);
    }
    MML_HIP(hipGetLastError());
    s->tail += n;
    return MML_OK;
}

// What the two assemble calls differ in.  The interval mode (sliced == 0) cuts frame i at [times[i], times[i + 1]): count + 1
// times; the offset mode takes up to `sliced` points from times[i]: count times.
struct UnionMode {
    const char* who;
    const uint64_t* times;
    int sliced;
    int n_times(int count) const { return sliced ? count : count + 1; }
};

int plan_args_ok(int count, const uint64_t* times, int n_times) {
    if (count < 1 || count > MML_UNION_BATCH_MAX || !times) return 0;
    for (int i = 0; i + 1 < n_times; ++i)
        if (times[i + 1] < times[i]) return 0;
    return 1;
}

// The checks of the assemble calls that need no device.
int union_check(mml_ctx* ctx, const UnionMode& m, mml_livox_stream* s, int first_slot, int count, const float* velo_xyzi, const int* vo,
                mml_union_frame* out) {
    const char* who = m.who;
    if (count < 1 || count > MML_UNION_BATCH_MAX) return mml_refuse(ctx, MML_ERR_INVALID, "%s: count = %d is outside 1 .. %d", who, count, MML_UNION_BATCH_MAX);
    if (first_slot < 0 || first_slot + count > ctx->B) return mml_refuse(ctx, MML_ERR_INVALID, "%s: slot range out of bounds", who);
    if (!s || !m.times || !vo || !out) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null argument", who);
    if (s->ctx != ctx) return mml_refuse(ctx, MML_ERR_INVALID, "%s: the stream belongs to another context", who);
    if (vo[0] < 0) return mml_refuse(ctx, MML_ERR_INVALID, "%s: frame 0: a negative offset", who);
    const int n_times = m.n_times(count);
    for (int i = 0; i < count; ++i) {
        if (i + 1 < n_times && m.times[i + 1] < m.times[i])
            return mml_refuse(ctx, MML_ERR_INVALID, m.sliced ? "%s: frame %d starts after the next one (starts must not decrease)"
                                                             : "%s: frame %d ends before it starts (stamps must not decrease)", who, i);
        if (vo[i + 1] < vo[i]) return mml_refuse(ctx, MML_ERR_INVALID, "%s: frame %d: velo_offsets must not decrease", who, i);
    }
    for (int i = 0; i < count; ++i)
        if (vo[i + 1] - vo[i] > ctx->cfg.max_velo_points)
            return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: frame %d: %d Velodyne rows exceed max_velo_points = %d", who, i, vo[i + 1] - vo[i],
                              ctx->cfg.max_velo_points);
    if (vo[count] > vo[0] && !velo_xyzi) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null cloud", who);
    return MML_OK;
}

// The device part of both assemble calls: one io block down, the mode's plan kernel, the gather, rows and verdict up.
int union_run(mml_ctx* ctx, const UnionMode& m, mml_livox_stream* s, int first_slot, int count, const float* velo_xyzi, const int* vo,
              const float* tf, mml_union_frame* out) {
    const size_t nv = (size_t)(vo[count] - vo[0]);
    int max_nv = 0;
    for (int i = 0; i < count; ++i) max_nv = vo[i + 1] - vo[i] > max_nv ? vo[i + 1] - vo[i] : max_nv;
    const UnionIo io((size_t)count);
    MmlUnionDev* u = mml_side<MmlUnionDev>(ctx, MML_SIDE_UNION);
    if (u->io.reserve(ctx, io.bytes) || u->velo.reserve(ctx, nv ? nv : 1)) {
        ctx->err = std::string(m.who) + ": the staging block could not be grown: " + ctx->err;
        return MML_ERR_HIP;
    }
    hipStream_t st = MML_STREAM(ctx);
    char *h = u->io.h, *g = u->io.d;
    memcpy(io.stamps.in(h), m.times, sizeof(uint64_t) * (size_t)m.n_times(count));  // (the field has room for count + 1)
    memcpy(io.voff.in(h), vo, io.voff.bytes());
    if (tf) memcpy(io.tf.in(h), tf, io.tf.bytes());
    const uint64_t* d_stamps = io.stamps.in(g);
    const int* d_voff = io.voff.in(g);
    const float* d_tf = tf ? io.tf.in(g) : nullptr;
    mml_union_frame* d_rows = io.rows.in(g);
    unsigned long long* d_verdict = io.verdict.in(g);
    // a frame holds at most max_livox_points points (the offset mode: sliced, which is no more), and no more than the queue does
    const long live = s->tail - s->front;
    const long room = m.sliced ? (long)m.sliced : (long)ctx->cfg.max_livox_points;
    const long most = live < room ? live : room;
    int gl = (int)((5 * most + 255) / 256), gv = (max_nv + 255) / 256;
    gl = gl < 1 ? 1 : (gl > UNION_GATHER_BLOCKS ? UNION_GATHER_BLOCKS : gl);
    gv = gv > UNION_GATHER_BLOCKS ? UNION_GATHER_BLOCKS : gv;
    {
        MmlStageScope t(ctx, m.sliced ? "union_offset_plan" : "union_plan");
        MML_HIP(hipMemcpyAsync(g, h, io.down_bytes, hipMemcpyHostToDevice, st));
        if (nv) MML_HIP(hipMemcpyAsync(u->velo.d, velo_xyzi + 4 * (size_t)vo[0], sizeof(float4) * nv, hipMemcpyHostToDevice, st));
        if (m.sliced)
            hipLaunchKernelGGL(k_union_plan_offset, dim3(1), dim3(256), 0, st, s->stamp[s->cur], s->base, s->front, s->tail, s->hs, count, d_stamps,
                               d_voff, first_slot, m.sliced, s->d_disorder, d_rows, d_verdict, ctx->d_n_in);
        else
            hipLaunchKernelGGL(k_union_plan, dim3(1), dim3(256), 0, st, s->stamp[s->cur], s->base, s->front, s->tail, s->hs, count, d_stamps, d_voff,
                               first_slot, ctx->cfg.max_livox_points, s->d_disorder, d_rows, d_verdict, ctx->d_n_in);
        MML_HIP(hipGetLastError());
    }
    {   // the call's ONE host synchronisation: the rows and the verdict in one copy
        MmlStageScope t(ctx, "union_gather");
        hipLaunchKernelGGL(k_union_gather, dim3((unsigned)(gl + gv), (unsigned)count), dim3(256), 0, st, d_rows, d_verdict, s->rec[s->cur],
                           s->stamp[s->cur], s->base, s->hs, d_stamps, u->velo.d, d_voff, d_tf, first_slot, gl,
                           ctx->velo_in, ctx->NV, reinterpret_cast<uint32_t*>(ctx->livox_in), ctx->NL);
        MML_HIP(hipGetLastError());
        MML_HIP(hipMemcpyAsync(io.rows.in(h), d_rows, io.up_bytes, hipMemcpyDeviceToHost, st));
    }
    MML_HIP(hipStreamSynchronize(st));
    unsigned long long bad = 0;
    memcpy(&bad, io.verdict.in(h), sizeof(bad));
    if (bad)
        return mml_refuse(ctx, MML_ERR_STATE, "%s: the stream holds %llu points older than the point before them; nothing was written", m.who, bad);
    memcpy(out, io.rows.in(h), io.rows.bytes());
    s->front = out[count - 1].front_after;  // (the offset mode moves it for NOT_REACHED too)
    for (int i = 0; i < count; ++i) {
        ctx->h_n_in[2 * (first_slot + i)] = vo[i + 1] - vo[i];
        ctx->raw_extracted[first_slot + i] = 0;
        ctx->h_n_in[2 * (first_slot + i) + 1] = out[i].status == MML_UNION_OK ? out[i].n_livox : 0;
    }
    return MML_OK;
}

}  // namespace

MmlLivoxView mml_livox_stream_view(const mml_livox_stream* s) {
    return MmlLivoxView{s->ctx, s->rec[s->cur], s->stamp[s->cur], s->base, s->front, s->tail, s->hs};
}

// mml_union_assemble: the checks that need no device (capi.hip calls them before it touches the slots) ...
int mml_union_check(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count, const uint64_t* stamps, const float* velo_xyzi,
                    const int* vo, mml_union_frame* out) {
    return union_check(ctx, UnionMode{"mml_union_assemble", stamps, 0}, s, first_slot, count, velo_xyzi, vo, out);
}
// ... and the device part, after them and CHECK_SLOTS.
int mml_union_run(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count, const uint64_t* stamps, const float* velo_xyzi, const int* vo,
                  const float* tf, mml_union_frame* out) {
    return union_run(ctx, UnionMode{"mml_union_assemble", stamps, 0}, s, first_slot, count, velo_xyzi, vo, tf, out);
}
// The same pair for mml_union_assemble_offset.
int mml_union_offset_check(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count, const uint64_t* starts, int sliced_points,
                           const float* velo_xyzi, const int* vo, mml_union_frame* out) {
    const char* who = "mml_union_assemble_offset";
    if (sliced_points < 1) return mml_refuse(ctx, MML_ERR_INVALID, "%s: sliced_points = %d is below 1", who, sliced_points);
    const int rc = union_check(ctx, UnionMode{who, starts, sliced_points}, s, first_slot, count, velo_xyzi, vo, out);
    if (rc != MML_OK) return rc;
    if (sliced_points > ctx->cfg.max_livox_points)
        return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: sliced_points = %d exceeds max_livox_points = %d", who, sliced_points, ctx->cfg.max_livox_points);
    return MML_OK;
}
int mml_union_offset_run(mml_ctx* ctx, mml_livox_stream* s, int first_slot, int count, const uint64_t* starts, int sliced_points,
                         const float* velo_xyzi, const int* vo, const float* tf, mml_union_frame* out) {
    return union_run(ctx, UnionMode{"mml_union_assemble_offset", starts, sliced_points}, s, first_slot, count, velo_xyzi, vo, tf, out);
}

extern "C" int mml_livox_stream_create(mml_ctx* ctx, long capacity_points, mml_livox_stream** out) {
    if (!ctx || !out) return MML_ERR_INVALID;
    *out = nullptr;
    // (5 * capacity dwords are indexed by int in the gather and the arrays are byte-addressed by size_t: 2^28 points is 5 GB of records)
    MML_REQUIRE(capacity_points >= 1 && capacity_points <= (1L << 28), MML_ERR_INVALID, "mml_livox_stream_create: capacity_points outside 1 .. 2^28");
    MML_HIP(hipSetDevice(ctx->device));
    mml_livox_stream* s = new mml_livox_stream();
    s->ctx = ctx;
    s->cap = capacity_points;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        e = s->mem.alloc(&s->rec[k], 5 * (size_t)capacity_points);
        if (e == hipSuccess) e = s->mem.alloc(&s->stamp[k], (size_t)capacity_points);
    }
    if (e == hipSuccess) e = s->mem.alloc(&s->d_disorder, 1);
    if (e == hipSuccess) e = s->mem.alloc_pinned(&s->h_disorder, 1);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_disorder, 0, sizeof(unsigned long long), MML_STREAM(ctx));
    if (e != hipSuccess) {
        ctx->err = std::string("mml_livox_stream_create: ") + hipGetErrorString(e);
        mml_livox_stream_destroy(s);
        return MML_ERR_HIP;
    }
    *out = s;
    return MML_OK;
}

extern "C" void mml_livox_stream_destroy(mml_livox_stream* s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(MML_STREAM(s->ctx));
    s->mem.release();
    delete s;
}

extern "C" int mml_livox_stream_reset(mml_livox_stream* s) {
    if (!s) return MML_ERR_INVALID;
    mml_ctx* ctx = s->ctx;
    MML_HIP(hipSetDevice(ctx->device));
    MML_HIP(hipMemsetAsync(s->d_disorder, 0, sizeof(unsigned long long), MML_STREAM(ctx)));
    s->base = s->front = s->tail = 0;
    s->hs = 0;
    s->have_hs = false;
    return MML_OK;
}

extern "C" int mml_livox_stream_push(mml_livox_stream* s, uint64_t timebase, const mml_livox_point* pts, int n) {
    return stream_push(s, "mml_livox_stream_push", timebase, pts, n, false);
}

extern "C" int mml_livox_stream_push_wire(mml_livox_stream* s, uint64_t timebase, const uint8_t* wire, int n) {
    return stream_push(s, "mml_livox_stream_push_wire", timebase, wire, n, true);
}

extern "C" int mml_livox_stream_state_get(mml_livox_stream* s, mml_livox_stream_state* out) {
    if (!s || !out) return MML_ERR_INVALID;
    mml_ctx* ctx = s->ctx;
    MML_HIP(hipSetDevice(ctx->device));
    MML_HIP(hipMemcpyAsync(s->h_disorder, s->d_disorder, sizeof(unsigned long long), hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    out->start_stamp = s->hs;
    out->front = s->front;
    out->tail = s->tail;
    out->disorder = (long)*s->h_disorder;
    return MML_OK;
}

extern "C" int mml_union_plan(const uint64_t* S, long front, long tail, uint64_t hs, int count, const uint64_t* stamps, int max_livox_points,
                              mml_union_frame* out) {
    if (!out || front < 0 || tail < front || (tail > front && !S) || !plan_args_ok(count, stamps, count + 1)) return MML_ERR_INVALID;
    for (long i = front + 1; i < tail; ++i)
        if (hs + S[i] < hs + S[i - 1]) return MML_ERR_STATE;
    long q = front;
    long lbs = mml_union_lower_bound(S, 0, front, tail, hs, stamps[0]);
    for (int i = 0; i < count; ++i) {
        const long lbe = mml_union_lower_bound(S, 0, front, tail, hs, stamps[i + 1]);
        q = mml_union_resolve(q, tail, lbs, lbe, max_livox_points, &out[i]);
        lbs = lbe;
    }
    return MML_OK;
}

extern "C" int mml_union_plan_offset(const uint64_t* S, long front, long tail, uint64_t hs, int count, const uint64_t* starts, int sliced_points,
                                     mml_union_frame* out) {
    if (!out || front < 0 || tail < front || (tail > front && !S) || sliced_points < 1 || !plan_args_ok(count, starts, count)) return MML_ERR_INVALID;
    for (long i = front + 1; i < tail; ++i)
        if (hs + S[i] < hs + S[i - 1]) return MML_ERR_STATE;
    long q = front;
    for (int i = 0; i < count; ++i)
        q = mml_union_resolve_offset(q, tail, mml_union_lower_bound(S, 0, front, tail, hs, starts[i]), sliced_points, &out[i]);
    return MML_OK;
}
