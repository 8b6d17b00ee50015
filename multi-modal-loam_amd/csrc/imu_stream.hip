// imu_stream.hip -- the pose node's IMU queue on the device (unionPoseEstimation.cpp):
//   :283-300  imuHandler's _imuMsgVector.push_back   mml_imu_stream_push: k_imu_push (the time-order count)
//   :307-395  fetchImuMsgs, n intervals per call     mml_imu_fetch_batch: k_imu_plan (which messages), k_imu_scan (where their
//                                                    rows go), k_imu_write (the rows, the synthesised one included)
//   :383-390  its trim of the queue                  mml_imu_stream_drop_before (host: the stamps are mirrored there)
//   :777-778  GyroIntegration                        k_imu_gyro
//   :798-799  PreIntegration                         k_imu_preintegrate (imu_preint.hip), launched unchanged on the packed rows
//   :779-780, :805-828  the frame prediction         mml_imu_predict_batch: k_imu_predict
// The stream is a flat array of messages, 7 doubles each (stamp, gyro xyz, accel xyz); message i (counted over everything
// ever pushed) sits at row i - base.  The cut, the gyro chain and the prediction are imu_fetch.h, shared with the host's
// mml_imu_fetch_host.  Compiled with -ffp-contract=off.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "imu_fetch.h"
#include "mml_internal.h"

struct mml_imu_stream {
    mml_ctx* ctx = nullptr;
    long cap = 0;
    double* msg[2] = {nullptr, nullptr};  // two arrays of cap messages: the live part moves from one to the other when the end is reached
    int cur = 0;
    long base = 0, front = 0, tail = 0;  // absolute message indices: row 0 of the current array, the queue's front, one past its last message
    unsigned long long* d_disorder = nullptr;  // time-order violations counted by k_imu_push
    unsigned long long* h_disorder = nullptr;  // pinned
    // The host's mirror of the stamps: message i at hstamp[i - hbase].  drop_before and the stamps of state_get read it, so
    // neither needs a kernel or a synchronisation (the alternative, a walk on the device, costs one read-back per trim).
    std::vector<double> hstamp;
    long hbase = 0;
    MmlFixed mem;  // owns the device and pinned buffers above
};

// The block of mml_imu_fetch_batch and the block of mml_imu_predict_batch, each with its pinned twin.  Grow-only; both calls
// drain the stream before they return, so reserve() never replaces a buffer in use.
struct MmlImuFetchDev {
    MmlStaging<char> io, pio;
    ~MmlImuFetchDev() {
        io.release();
        pio.release();
    }
};

namespace {

constexpr int IMU_SCAN_THREADS = 1024;
constexpr long IMU_STREAM_MAX = 1L << 24;  // messages: a count fits an int, 7 * rows * 8 bytes a size_t with room

// The n messages at rows [pos, pos + n): each compared with the one before it in the queue (has_prev: row pos - 1 is live).
__global__ __launch_bounds__(256) void k_imu_push(const double* __restrict__ msg, long pos, int n, int has_prev,
                                                  unsigned long long* __restrict__ disorder) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    if (j == 0 && !has_prev) return;
    if (msg[7 * (size_t)(pos + j)] < msg[7 * (size_t)(pos + j - 1)]) atomicAdd(disorder, 1ull);
}

// A lane per interval: the two searches of one interval depend on nothing another lane loads.  A stream with time-order
// violations gets no rows at all (the searches mean nothing on it); k_imu_scan reports it.
__global__ __launch_bounds__(256) void k_imu_plan(const double* __restrict__ msg, long base, long front, long tail, int n,
                                                  const double* __restrict__ ts, const double* __restrict__ te,
                                                  const unsigned long long* __restrict__ disorder, mml_imu_interval* __restrict__ rows,
                                                  int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    mml_imu_interval r;
    imu_fetch_plan(msg, base, front, tail, ts[i], te[i], &r);
    rows[i] = r;
    counts[i] = *disorder ? 0 : r.n;
}

// ONE workgroup: the exclusive scan of the counts.  offsets (n + 1, what the caller gets) saturate at INT_MAX; koff (n + 1, what
// the kernels after this one index the packed rows with) equals offsets when the total fits `cap` rows and is all zero
// otherwise, so that no kernel writes or reads a row then.  verdict: violations | total.
__global__ __launch_bounds__(IMU_SCAN_THREADS) void k_imu_scan(const int* __restrict__ counts, int n, long cap,
                                                               const unsigned long long* __restrict__ disorder, int* __restrict__ offsets,
                                                               int* __restrict__ koff, unsigned long long* __restrict__ verdict) {
    __shared__ long s_sum[IMU_SCAN_THREADS];
    const int t = threadIdx.x;
    const int per = (n + IMU_SCAN_THREADS - 1) / IMU_SCAN_THREADS;
    const int i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
    long mine = 0;
    for (int i = i0; i < i1; ++i) mine += counts[i];
    s_sum[t] = mine;
    __syncthreads();
    for (int d = 1; d < IMU_SCAN_THREADS; d <<= 1) {  // inclusive scan of the threads' sums
        const long add = t >= d ? s_sum[t - d] : 0;
        __syncthreads();
        s_sum[t] += add;
        __syncthreads();
    }
    const long total = s_sum[IMU_SCAN_THREADS - 1];
    const unsigned long long bad = *disorder;
    const bool fits = !bad && total <= cap;
    long run = s_sum[t] - mine;
    for (int i = i0; i < i1; ++i) {
        const int o = run > (long)INT_MAX ? INT_MAX : (int)run;
        offsets[i] = o;
        koff[i] = fits ? o : 0;
        run += counts[i];
    }
    if (t == 0) {
        const int o = total > (long)INT_MAX ? INT_MAX : (int)total;
        offsets[n] = o;
        koff[n] = fits ? o : 0;
        verdict[0] = bad;
        verdict[1] = (unsigned long long)total;
    }
}

// A wavefront per interval, its lanes striding the interval's rows; the last row of an interpolated interval is synthesised.
__global__ __launch_bounds__(256) void k_imu_write(const double* __restrict__ msg, long base, int n, const mml_imu_interval* __restrict__ rows,
                                                   const int* __restrict__ koff, const double* __restrict__ ts, const double* __restrict__ te,
                                                   double* __restrict__ out) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const int o = koff[i], cnt = koff[i + 1] - o;  // rows[i].n, or 0 when the rows are not to be written
    const mml_imu_interval r = rows[i];
    const double start = ts[i], end = te[i];
    for (int k = lane; k < cnt; k += 64) {
        double row[7];
        imu_fetch_row(msg, base, r.first, r.n, r.interpolated, start, end, k, row);
        double* dst = out + 7 * (size_t)(o + k);
        for (int c = 0; c < 7; ++c) dst[c] = row[c];
    }
}

// A lane per interval: the gyro chain is serial in the interval's rows.
__global__ __launch_bounds__(64) void k_imu_gyro(const double* __restrict__ packed, const int* __restrict__ koff, int n, double* __restrict__ dq) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double q[4];
    imu_fetch_gyro(packed + 7 * (size_t)koff[i], koff[i + 1] - koff[i], q);
    for (int k = 0; k < 4; ++k) dq[4 * (size_t)i + k] = q[k];
}

// A lane per interval.  pd: n x 10 = the pre-integration's dq (4), dp (3), dv (3); a group whose input is null is left out.
__global__ __launch_bounds__(64) void k_imu_predict(int n, const double* __restrict__ ex, const double* __restrict__ prev, const double* __restrict__ pd,
                                                    const double* __restrict__ gq, double* __restrict__ state, double* __restrict__ dRl,
                                                    double* __restrict__ dtl, double* __restrict__ gRb, double* __restrict__ gRl) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const ImuExtrinsic e = imu_extrinsic(ex);
    const size_t u = (size_t)i;
    if (prev) imu_predict_lio(prev + 10 * u, pd + 10 * u, pd + 10 * u + 4, pd + 10 * u + 7, e, state + 10 * u, dRl + 9 * u, dtl + 3 * u);
    if (gq) imu_predict_gyro(gq + 4 * u, e, gRb + 9 * u, gRl + 9 * u);
}

// Room for n more messages: when the current array's end would be passed, the live part moves to the front of the other array
// (different allocations, ordered on the stream like everything else).
int imu_make_room(mml_imu_stream* s, int n) {
    mml_ctx* ctx = s->ctx;
    if (s->tail - s->base + n <= s->cap) return MML_OK;
    const long live = s->tail - s->front, at = s->front - s->base;
    if (live > 0)
        MML_HIP(hipMemcpyAsync(s->msg[1 - s->cur], s->msg[s->cur] + 7 * (size_t)at, 56 * (size_t)live, hipMemcpyDeviceToDevice, MML_STREAM(ctx)));
    s->cur = 1 - s->cur;
    s->base = s->front;
    return MML_OK;
}

// The checks of the two fetch calls that need neither a stream nor a device.
int fetch_check(mml_ctx* ctx, const char* who, int n, const double* ts, const double* te, const double* bg, const double* ba,
                const mml_imu_interval* rows, const int* offsets, long cap, const mml_imu_preint* pre) {
    if (n < 1 || n > MML_IMU_FETCH_BATCH_MAX) return mml_refuse(ctx, MML_ERR_INVALID, "%s: n = %d is outside 1 .. %d", who, n, MML_IMU_FETCH_BATCH_MAX);
    if (!ts || !te || !rows || !offsets) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null argument", who);
    if ((bg == nullptr) != (ba == nullptr)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: bg and ba must both be given or both be null", who);
    if (pre && !bg) return mml_refuse(ctx, MML_ERR_INVALID, "%s: pre needs the biases", who);
    if (cap < 0) return mml_refuse(ctx, MML_ERR_INVALID, "%s: sample_capacity = %ld is negative", who, cap);
    for (int i = 0; i < n; ++i)
        if (!isfinite(ts[i]) || !isfinite(te[i])) return mml_refuse(ctx, MML_ERR_INVALID, "%s: interval %d: a time is not finite", who, i);
    return MML_OK;
}

// io block: what goes down in one copy, the device's own scratch, then what comes back in one copy (the packed rows last, so
// that a call without `samples` does not move them)
struct FetchIo {
    MmlCarve<256> c;
    MmlField<double> ts, te, bias;
    MmlField<int> counts, koff;
    MmlField<mml_imu_interval> rows;
    MmlField<int> offsets;
    MmlField<unsigned long long> verdict;
    MmlField<double> dq;
    MmlField<mml_imu_preint> pre;
    MmlField<double> packed;
    FetchIo(size_t n, bool want_pre, bool want_dq, size_t cap_rows)
        : ts(c.take<double>(n)), te(c.take<double>(n)), bias(c.take<double>(want_pre ? 6 * n : 0)), counts(c.take<int>(n)),
          koff(c.take<int>(n + 1)), rows(c.take<mml_imu_interval>(n)), offsets(c.take<int>(n + 1)), verdict(c.take<unsigned long long>(2)),
          dq(c.take<double>(want_dq ? 4 * n : 0)), pre(c.take<mml_imu_preint>(want_pre ? n : 0)), packed(c.take<double>(7 * cap_rows)) {}
    size_t down_bytes() const { return counts.off; }
};

}  // namespace

extern "C" int mml_imu_stream_create(mml_ctx* ctx, long capacity_msgs, mml_imu_stream** out) {
    if (!ctx || !out) return MML_ERR_INVALID;
    *out = nullptr;
    if (capacity_msgs < 1 || capacity_msgs > IMU_STREAM_MAX)
        return mml_refuse(ctx, MML_ERR_INVALID, "mml_imu_stream_create: capacity_msgs = %ld is outside 1 .. 2^24", capacity_msgs);
    MML_HIP(hipSetDevice(ctx->device));
    mml_imu_stream* s = new mml_imu_stream();
    s->ctx = ctx;
    s->cap = capacity_msgs;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; ++k) e = s->mem.alloc(&s->msg[k], 7 * (size_t)capacity_msgs);
    if (e == hipSuccess) e = s->mem.alloc(&s->d_disorder, 1);
    if (e == hipSuccess) e = s->mem.alloc_pinned(&s->h_disorder, 1);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_disorder, 0, sizeof(unsigned long long), MML_STREAM(ctx));
    if (e != hipSuccess) {
        ctx->err = std::string("mml_imu_stream_create: ") + hipGetErrorString(e);
        mml_imu_stream_destroy(s);
        return MML_ERR_HIP;
    }
    *out = s;
    return MML_OK;
}

extern "C" void mml_imu_stream_destroy(mml_imu_stream* s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(MML_STREAM(s->ctx));
    s->mem.release();
    delete s;
}

extern "C" int mml_imu_stream_reset(mml_imu_stream* s) {
    if (!s) return MML_ERR_INVALID;
    mml_ctx* ctx = s->ctx;
    MML_HIP(hipSetDevice(ctx->device));
    MML_HIP(hipMemsetAsync(s->d_disorder, 0, sizeof(unsigned long long), MML_STREAM(ctx)));
    s->base = s->front = s->tail = s->hbase = 0;
    s->hstamp.clear();
    return MML_OK;
}

extern "C" int mml_imu_stream_push(mml_imu_stream* s, const double* msgs, int n) {
    if (!s) return MML_ERR_INVALID;
    mml_ctx* ctx = s->ctx;
    const char* who = "mml_imu_stream_push";
    if (n < 0 || (n > 0 && !msgs)) return mml_refuse(ctx, MML_ERR_INVALID, "%s: %s", who, n < 0 ? "negative message count" : "null message buffer");
    if ((s->tail - s->front) + n > s->cap)
        return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: %ld live messages + %d exceed capacity_msgs = %ld", who, s->tail - s->front, n, s->cap);
    for (int j = 0; j < n; ++j)
        if (!isfinite(msgs[7 * (size_t)j])) return mml_refuse(ctx, MML_ERR_INVALID, "%s: message %d: its stamp is not finite", who, j);
    if (n == 0) return MML_OK;
    MML_HIP(hipSetDevice(ctx->device));
    int rc = imu_make_room(s, n);
    if (rc != MML_OK) return rc;
    hipStream_t st = MML_STREAM(ctx);
    const long pos = s->tail - s->base;
    double* msg = s->msg[s->cur];
    MML_HIP(hipMemcpyAsync(msg + 7 * (size_t)pos, msgs, 56 * (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_imu_push, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, msg, pos, n, s->tail > s->front ? 1 : 0, s->d_disorder);
    MML_HIP(hipGetLastError());
    if (s->front - s->hbase > (long)s->hstamp.size() / 2) {  // the mirror forgets what the queue dropped
        s->hstamp.erase(s->hstamp.begin(), s->hstamp.begin() + (s->front - s->hbase));
        s->hbase = s->front;
    }
    for (int j = 0; j < n; ++j) s->hstamp.push_back(msgs[7 * (size_t)j]);
    s->tail += n;
    return MML_OK;
}

extern "C" int mml_imu_stream_drop_before(mml_imu_stream* s, double t, long keep_min) {
    if (!s) return MML_ERR_INVALID;
    if (keep_min < 0 || t != t) return mml_refuse(s->ctx, MML_ERR_INVALID, "mml_imu_stream_drop_before: keep_min < 0 or t is not a number");
    while (s->tail - s->front > keep_min && s->hstamp[(size_t)(s->front - s->hbase)] < t) ++s->front;  // :386-390
    return MML_OK;
}

extern "C" int mml_imu_stream_state_get(mml_imu_stream* s, mml_imu_stream_state* out) {
    if (!s || !out) return MML_ERR_INVALID;
    mml_ctx* ctx = s->ctx;
    MML_HIP(hipSetDevice(ctx->device));
    MML_HIP(hipMemcpyAsync(s->h_disorder, s->d_disorder, sizeof(unsigned long long), hipMemcpyDeviceToHost, MML_STREAM(ctx)));
    MML_HIP(hipStreamSynchronize(MML_STREAM(ctx)));
    out->front = s->front;
    out->tail = s->tail;
    out->disorder = (long)*s->h_disorder;
    const bool live = s->tail > s->front;
    out->first_stamp = live ? s->hstamp[(size_t)(s->front - s->hbase)] : 0.0;
    out->last_stamp = live ? s->hstamp[(size_t)(s->tail - 1 - s->hbase)] : 0.0;
    return MML_OK;
}

extern "C" int mml_imu_fetch_batch(mml_ctx* ctx, mml_imu_stream* s, int n, const double* t_start, const double* t_end, const double* bg,
                                   const double* ba, mml_imu_interval* rows, int* offsets, double* samples, long sample_capacity,
                                   mml_imu_preint* pre, double* dq) {
    const char* who = "mml_imu_fetch_batch";
    if (!ctx) return MML_ERR_INVALID;
    if (!s) return mml_refuse(ctx, MML_ERR_INVALID, "%s: a null stream", who);
    if (s->ctx != ctx) return mml_refuse(ctx, MML_ERR_INVALID, "%s: the stream belongs to another context", who);
    int rc = fetch_check(ctx, who, n, t_start, t_end, bg, ba, rows, offsets, sample_capacity, pre);
    if (rc != MML_OK) return rc;
    MML_HIP(hipSetDevice(ctx->device));
    const bool need_rows = samples || pre || dq;
    const long live = s->tail - s->front;
    // rows the device block holds: no interval has more rows than the queue has live messages
    long cap_rows = 0;
    if (need_rows) {
        cap_rows = sample_capacity < (long)n * live ? sample_capacity : (long)n * live;
        cap_rows = cap_rows > (long)INT_MAX ? (long)INT_MAX : cap_rows;
    }
    const FetchIo io((size_t)n, pre != nullptr, dq != nullptr, (size_t)(cap_rows > 0 ? cap_rows : 1));
    MmlImuFetchDev* d = mml_side<MmlImuFetchDev>(ctx, MML_SIDE_IMU_FETCH);
    if (d->io.reserve(ctx, io.c.bytes())) {
        ctx->err = std::string(who) + ": the block could not be grown: " + ctx->err;
        return MML_ERR_HIP;
    }
    char *h = d->io.h, *g = d->io.d;
    memcpy(io.ts.in(h), t_start, io.ts.bytes());
    memcpy(io.te.in(h), t_end, io.te.bytes());
    if (pre) {
        double* hb = io.bias.in(h);
        for (int i = 0; i < n; ++i) {
            memcpy(hb + 6 * (size_t)i, bg + 3 * (size_t)i, sizeof(double) * 3);
            memcpy(hb + 6 * (size_t)i + 3, ba + 3 * (size_t)i, sizeof(double) * 3);
        }
    }
    hipStream_t st = MML_STREAM(ctx);
    const double* msg = s->msg[s->cur];
    const size_t up_end = samples ? io.packed.off + 56 * (size_t)cap_rows : io.pre.end() > io.dq.end() ? io.pre.end() : io.dq.end();
    {
        MmlStageScope t(ctx, "imu_fetch_plan");
        MML_HIP(hipMemcpyAsync(g, h, io.down_bytes(), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_imu_plan, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, msg, s->base, s->front, s->tail, n, io.ts.in(g), io.te.in(g),
                           s->d_disorder, io.rows.in(g), io.counts.in(g));
        hipLaunchKernelGGL(k_imu_scan, dim3(1), dim3(IMU_SCAN_THREADS), 0, st, io.counts.in(g), n, need_rows ? cap_rows : LONG_MAX, s->d_disorder,
                           io.offsets.in(g), io.koff.in(g), io.verdict.in(g));
        MML_HIP(hipGetLastError());
    }
    if (need_rows) {
        MmlStageScope t(ctx, "imu_fetch_rows");
        hipLaunchKernelGGL(k_imu_write, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, msg, s->base, n, io.rows.in(g), io.koff.in(g), io.ts.in(g),
                           io.te.in(g), io.packed.in(g));
        MML_HIP(hipGetLastError());
        if (pre) {
            rc = mml_launch_imu_preintegrate(ctx, n, io.packed.in(g), io.koff.in(g), io.bias.in(g), io.pre.in(g));
            if (rc != MML_OK) return rc;
        }
        if (dq) {
            hipLaunchKernelGGL(k_imu_gyro, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, io.packed.in(g), io.koff.in(g), n, io.dq.in(g));
            MML_HIP(hipGetLastError());
        }
    }
    // the call's ONE read-back and ONE host synchronisation
    MML_HIP(hipMemcpyAsync(io.rows.in(h), io.rows.in(g), up_end - io.rows.off, hipMemcpyDeviceToHost, st));
    MML_HIP(hipStreamSynchronize(st));
    unsigned long long verdict[2];
    memcpy(verdict, io.verdict.in(h), sizeof(verdict));
    if (verdict[0])
        return mml_refuse(ctx, MML_ERR_STATE, "%s: the stream holds %llu messages older than the message before them; nothing was written", who,
                          verdict[0]);
    memcpy(rows, io.rows.in(h), io.rows.bytes());
    memcpy(offsets, io.offsets.in(h), io.offsets.bytes());
    const unsigned long long total = verdict[1];
    if (need_rows && total > (unsigned long long)sample_capacity)
        return mml_refuse(ctx, MML_ERR_CAPACITY, "%s: %llu rows exceed sample_capacity = %ld", who, total, sample_capacity);
    if (!need_rows) return MML_OK;
    if (samples && total) memcpy(samples, io.packed.in(h), 56 * (size_t)total);
    if (pre) memcpy(pre, io.pre.in(h), io.pre.bytes());
    if (dq) memcpy(dq, io.dq.in(h), io.dq.bytes());
    return MML_OK;
}

extern "C" int mml_imu_fetch_host(const double* msgs, long n_msgs, int n, const double* t_start, const double* t_end, const double* bg,
                                  const double* ba, mml_imu_interval* rows, int* offsets, double* samples, long sample_capacity,
                                  mml_imu_preint* pre, double* dq) {
    mml_ctx* ctx = nullptr;
    const char* who = "mml_imu_fetch_host";
    if (n_msgs < 0 || n_msgs > IMU_STREAM_MAX || (n_msgs > 0 && !msgs)) return MML_ERR_INVALID;
    int rc = fetch_check(ctx, who, n, t_start, t_end, bg, ba, rows, offsets, sample_capacity, pre);
    if (rc != MML_OK) return rc;
    for (long i = 0; i < n_msgs; ++i)
        if (!isfinite(msgs[7 * (size_t)i])) return MML_ERR_INVALID;
    for (long i = 1; i < n_msgs; ++i)
        if (msgs[7 * (size_t)i] < msgs[7 * (size_t)(i - 1)]) return MML_ERR_STATE;
    const bool need_rows = samples || pre || dq;
    std::vector<mml_imu_interval> r((size_t)n);
    std::vector<int> off((size_t)n + 1);
    long total = 0;
    for (int i = 0; i < n; ++i) {
        imu_fetch_plan(msgs, 0, 0, n_msgs, t_start[i], t_end[i], &r[(size_t)i]);
        off[(size_t)i] = total > (long)INT_MAX ? INT_MAX : (int)total;
        total += r[(size_t)i].n;
    }
    off[(size_t)n] = total > (long)INT_MAX ? INT_MAX : (int)total;
    memcpy(rows, r.data(), sizeof(mml_imu_interval) * (size_t)n);
    memcpy(offsets, off.data(), sizeof(int) * ((size_t)n + 1));
    if (!need_rows) return MML_OK;
    if (total > sample_capacity) return MML_ERR_CAPACITY;
    std::vector<double> own;
    double* packed = samples;
    if (!packed) {
        own.resize(7 * (size_t)(total ? total : 1));
        packed = own.data();
    }
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < r[(size_t)i].n; ++k)
            imu_fetch_row(msgs, 0, r[(size_t)i].first, r[(size_t)i].n, r[(size_t)i].interpolated, t_start[i], t_end[i], k,
                          packed + 7 * (size_t)(off[(size_t)i] + k));
    if (pre && (rc = mml_imu_preintegrate_batch(nullptr, n, packed, off.data(), bg, ba, pre)) != MML_OK) return rc;
    if (dq)
        for (int i = 0; i < n; ++i) imu_fetch_gyro(packed + 7 * (size_t)off[(size_t)i], r[(size_t)i].n, dq + 4 * (size_t)i);
    return MML_OK;
}

extern "C" int mml_imu_predict_batch(mml_ctx* ctx, int n, const double* exTlb, const double* prev, const mml_imu_preint* pre, double* state,
                                     double* delta_Rl, double* delta_tl, const double* dq, double* gyro_Rb, double* gyro_Rl) {
    const char* who = "mml_imu_predict_batch";
    if (n < 1 || n > MML_IMU_FETCH_BATCH_MAX) return mml_refuse(ctx, MML_ERR_INVALID, "%s: n = %d is outside 1 .. %d", who, n, MML_IMU_FETCH_BATCH_MAX);
    const int lio_given = (prev != nullptr) + (pre != nullptr) + (state != nullptr) + (delta_Rl != nullptr) + (delta_tl != nullptr);
    const int gyro_given = (dq != nullptr) + (gyro_Rb != nullptr) + (gyro_Rl != nullptr);
    if (!exTlb) return mml_refuse(ctx, MML_ERR_INVALID, "%s: exTlb is null", who);
    if ((lio_given != 0 && lio_given != 5) || (gyro_given != 0 && gyro_given != 3) || lio_given + gyro_given == 0)
        return mml_refuse(ctx, MML_ERR_INVALID, "%s: a group of arguments is given in part, or none is given", who);
    const bool lio = lio_given != 0, gyro = gyro_given != 0;
    const size_t N = (size_t)n;
    if (!ctx) {
        const ImuExtrinsic e = imu_extrinsic(exTlb);
        for (size_t i = 0; i < N; ++i) {
            if (lio) imu_predict_lio(prev + 10 * i, pre[i].dq, pre[i].dp, pre[i].dv, e, state + 10 * i, delta_Rl + 9 * i, delta_tl + 3 * i);
            if (gyro) imu_predict_gyro(dq + 4 * i, e, gyro_Rb + 9 * i, gyro_Rl + 9 * i);
        }
        return MML_OK;
    }
    MML_HIP(hipSetDevice(ctx->device));
    MmlCarve<256> c;
    const auto f_ex = c.take<double>(16), f_prev = c.take<double>(lio ? 10 * N : 0), f_pd = c.take<double>(lio ? 10 * N : 0),
               f_gq = c.take<double>(gyro ? 4 * N : 0);
    const auto f_state = c.take<double>(lio ? 10 * N : 0), f_dRl = c.take<double>(lio ? 9 * N : 0), f_dtl = c.take<double>(lio ? 3 * N : 0),
               f_gRb = c.take<double>(gyro ? 9 * N : 0), f_gRl = c.take<double>(gyro ? 9 * N : 0);
    MmlImuFetchDev* d = mml_side<MmlImuFetchDev>(ctx, MML_SIDE_IMU_FETCH);
    if (d->pio.reserve(ctx, c.bytes())) {
        ctx->err = std::string(who) + ": the block could not be grown: " + ctx->err;
        return MML_ERR_HIP;
    }
    char *h = d->pio.h, *g = d->pio.d;
    memcpy(f_ex.in(h), exTlb, f_ex.bytes());
    if (lio) {
        memcpy(f_prev.in(h), prev, f_prev.bytes());
        double* pd = f_pd.in(h);
        for (size_t i = 0; i < N; ++i) {
            memcpy(pd + 10 * i, pre[i].dq, sizeof(double) * 4);
            memcpy(pd + 10 * i + 4, pre[i].dp, sizeof(double) * 3);
            memcpy(pd + 10 * i + 7, pre[i].dv, sizeof(double) * 3);
        }
    }
    if (gyro) memcpy(f_gq.in(h), dq, f_gq.bytes());
    hipStream_t st = MML_STREAM(ctx);
    const size_t down = f_state.off, up0 = f_state.off;  // (a field without elements still knows where it would start)
    MmlStageScope t(ctx, "imu_predict");
    MML_HIP(hipMemcpyAsync(g, h, down, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_imu_predict, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, f_ex.in(g), lio ? f_prev.in(g) : nullptr,
                       lio ? f_pd.in(g) : nullptr, gyro ? f_gq.in(g) : nullptr, f_state.in(g), f_dRl.in(g), f_dtl.in(g), f_gRb.in(g), f_gRl.in(g));
    MML_HIP(hipGetLastError());
    MML_HIP(hipMemcpyAsync(h + up0, g + up0, c.last - up0, hipMemcpyDeviceToHost, st));
    MML_HIP(hipStreamSynchronize(st));
    if (lio) {
        memcpy(state, f_state.in(h), f_state.bytes());
        memcpy(delta_Rl, f_dRl.in(h), f_dRl.bytes());
        memcpy(delta_tl, f_dtl.in(h), f_dtl.bytes());
    }
    if (gyro) {
        memcpy(gyro_Rb, f_gRb.in(h), f_gRb.bytes());
        memcpy(gyro_Rl, f_gRl.in(h), f_gRl.bytes());
    }
    return MML_OK;
}
