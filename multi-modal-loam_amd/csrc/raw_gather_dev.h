// raw_gather_dev.h -- the walk over a sensor's RAW scan that finds every point's place in the slot's line-bucketed storage, shared
// by the two kernels that hand out clouds in raw order: k_gicp_gather_raw (gicp.hip: the surf clouds the refresh aligns) and
// k_feature_gather (capi.hip: the four feature clouds of the union_cloud message).
//
// Storage: block-major (blocks of blk_points raw points; one block = the whole scan after the three-pass bucketing), line-bucketed
// inside a block, raw order inside a (block, line) segment; segment (blk, key) starts at flat[blk * nkeys + key].  The bucketed
// position of raw point i is therefore its segment's start plus the number of earlier points of its block that carry its line id.
//
// One workgroup of RG_THREADS threads per (sensor, slot) takes RG_THREADS consecutive raw points per round (blk_points is a
// multiple of that: a round never straddles blocks).  A wavefront ranks its 64 points by ballots, leaves its per-line counts in its
// own row of an LDS table, and a point adds the rows of the wavefronts before its own and the per-line running count of the
// earlier rounds (reset at every block boundary).  classify(p) -- which reads the label byte at the position -- sorts the point
// into output cloud 0, 1 or none (-1); the output index is the cloud's cursor (kept by every thread in a register: the sum of the
// wavefronts' counts of the earlier rounds) plus the counts of the wavefronts before + the rank inside the wavefront, so the
// takers of a wavefront hold consecutive indices and emit(cloud, index, i, p, key) stores contiguous records.  Two barriers per
// round, one more at a block boundary.  n_out: the two clouds' sizes, in every thread.
#ifndef MML_RAW_GATHER_DEV_H
#define MML_RAW_GATHER_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int RG_THREADS = 1024;
constexpr int RG_WAVES = RG_THREADS / 64;
constexpr int RG_KEYS = 256;  // line ids are bytes; 254 and 255 mark raw points that were dropped before the bucketing

struct RawGatherSrc {
    const uint8_t* raw_line;  // line id per raw point of this sensor
    const int* flat;          // this (slot, sensor)'s segment starts
    int n, nkeys, blk_points;
    int flat_n, n_pos;        // entries of flat | positions of the slot's storage: no index derived from device tables goes past them
};

template <class Classify, class Emit>
__device__ __forceinline__ void raw_gather_walk(const RawGatherSrc& S, Classify classify, Emit emit, int n_out[2]) {
    __shared__ int s_run[RG_KEYS];            // points of each line in the earlier rounds of the current block
    __shared__ int s_seg[RG_KEYS];            // start of each line's segment of the current block
    __shared__ int s_wcnt[RG_WAVES][RG_KEYS];  // this round: points of each line per wavefront
    __shared__ int s_wout[RG_WAVES];          // this round: takers per wavefront, cloud 0 | cloud 1 << 16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int nk = S.nkeys < RG_KEYS - 2 ? S.nkeys : RG_KEYS - 2;
    n_out[0] = n_out[1] = 0;
    int key_next = tid < S.n ? (int)S.raw_line[tid] : 255;
    for (int i0 = 0; i0 < S.n; i0 += RG_THREADS) {
        const int i = i0 + tid, key = key_next;
        key_next = i + RG_THREADS < S.n ? (int)S.raw_line[i + RG_THREADS] : 255;  // (on its way while this round ranks)
        if (i0 % S.blk_points == 0) {
            __syncthreads();  // (the round before still adds to s_run)
            if (tid < nk) {
                s_run[tid] = 0;
                const int f = (i0 / S.blk_points) * S.nkeys + tid;
                s_seg[tid] = S.flat[f < S.flat_n ? f : S.flat_n - 1];
            }
        }
        const bool valid = key < nk;
        unsigned long long eq = __ballot(valid);  // lanes holding the same line id as mine
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (key >> bit) & 1;
            const unsigned long long bm = __ballot(valid && set);
            eq &= set ? bm : ~bm;
        }
        const bool first = valid && (eq & lt) == 0;
        for (int k = lane; k < nk; k += 64) s_wcnt[wave][k] = 0;
        __builtin_amdgcn_wave_barrier();
        if (first) s_wcnt[wave][key] = __popcll(eq);
        __syncthreads();
        int c = -1, p = 0;
        if (valid) {
            int pos = s_run[key] + __popcll(eq & lt);
            for (int w = 0; w < wave; ++w) pos += s_wcnt[w][key];
            p = s_seg[key] + pos;
            p = p < 0 ? 0 : (p < S.n_pos ? p : S.n_pos - 1);
            c = classify(p);
        }
        const unsigned long long m0 = __ballot(c == 0), m1 = __ballot(c == 1);
        if (lane == 0) s_wout[wave] = __popcll(m0) | (__popcll(m1) << 16);
        __syncthreads();
        if (first) atomicAdd(&s_run[key], __popcll(eq));  // (read again only behind the next round's first barrier)
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < RG_WAVES; ++w) {
            const int v = s_wout[w];
            all += v;
            before += w < wave ? v : 0;
        }
        if (c >= 0) emit(c, (c ? n_out[1] : n_out[0]) + ((before >> (16 * c)) & 0xffff) + __popcll((c ? m1 : m0) & lt), i, p, key);
        n_out[0] += all & 0xffff;
        n_out[1] += all >> 16;
    }
}

#endif
