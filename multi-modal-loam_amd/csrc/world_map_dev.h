// world_map_dev.h -- what the world map's kernels in more than one translation unit share (world_map.hip, world_map_assoc.hip,
// world_map_score.hip): the per-wave counter add, the read-only probe, the association's candidate walk, the moment arrays, the
// surfel record of one voxel and the entry of the surfel cache made from it.  Device only; include inside an anonymous namespace
// of the translation unit, behind eig3_dev.h and world_map_assoc.h.
#ifndef MML_WORLD_MAP_DEV_H
#define MML_WORLD_MAP_DEV_H

#include "world_map_assoc.h"

// one add per wave of the lanes for which `pred` holds
__device__ __forceinline__ void wm_count(int* counter, bool pred) {
    const unsigned long long b = __ballot(pred);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(counter, __popcll(b));
}

// where `key` sits in the table, or -1: the probe ends at the key or at the first free position (there always is one: the table
// holds at most half as many voxels as it has positions)
__device__ __forceinline__ long long wm_find(const unsigned long long* __restrict__ tab, unsigned long long slots, unsigned long long key) {
    unsigned long long h = mml_wm_hash(key, slots);
    for (unsigned long long step = 0; step < slots; ++step) {
        const unsigned long long k = tab[h];
        if (k == key) return (long long)h;
        if (k == MML_WM_EMPTY) return -1;
        h = (h + 1) & (slots - 1);
    }
    return -1;
}

// The association's walk over the candidates of a world point w in voxel (vi, vj, vk) of map `map` (world_map_assoc.h: which
// voxels, which of them wins), for k_wm_associate and k_wm_score alike: the up to 27 probes run in three groups of nine (one k
// layer each) -- the nine hash positions are computed, their first key loads are issued together, and only a probe that met
// another voxel's key walks on (wm_find, from its second position on).  The table is only read.
__device__ __forceinline__ void wm_probe27(const unsigned long long* keys, unsigned long long slots, const float4* sum, const int* count, int map,
                                           int nb, int min_points, int vi, int vj, int vk, float wx, float wy, float wz, MmlWmaBest& best) {
    for (int dk = -1; dk <= 1; ++dk) {
        if (!nb && dk != 0) continue;
        unsigned long long key[9], k0[9];
        unsigned h[9];
        bool use[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const int di = c % 3 - 1, dj = c / 3 - 1;
            key[c] = 0;
            use[c] = (nb || (di == 0 && dj == 0)) && mml_wma_candidate(map, vi + di, vj + dj, vk + dk, key[c]);
            h[c] = use[c] ? (unsigned)mml_wm_hash(key[c], slots) : 0u;
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) k0[c] = use[c] ? keys[h[c]] : MML_WM_EMPTY;  // the nine first loads, none waits for another
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            if (!use[c]) continue;
            long long at = -1;
            unsigned long long k = k0[c], hh = h[c];
            for (unsigned long long step = 1;; ++step) {  // (wm_find, from its second position on)
                if (k == key[c]) {
                    at = (long long)hh;
                    break;
                }
                if (k == MML_WM_EMPTY || step >= slots) break;
                hh = (hh + 1) & (slots - 1);
                k = keys[hh];
            }
            if (at < 0) continue;
            const int n = count[at];
            if (n < min_points) continue;
            const float4 s = sum[at];
            const MmlWmAcc a = {s.x, s.y, s.z, s.w, n};
            float cen[4];
            mml_wm_centroid(a, cen);
            mml_wma_offer(best, mml_wma_r2(wx, wy, wz, cen[0], cen[1], cen[2]), key[c], at, n, cen[0], cen[1], cen[2]);
        }
    }
}

// the three moment arrays of a surfel map; null in a plain map
struct WmMom {
    float4 *m0, *m1, *m2;
};
__device__ __forceinline__ MmlWmMoments wm_moments(const float4& a, const float4& b, const float4& c) {
    return MmlWmMoments{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
}

// The surfel record of one voxel of np >= 3 points with the moments m, 8 floats: the normal (the eigenvector of the smallest
// eigenvalue, turned towards the view sum), the eigenvalues ascending, planarity and linearity.  (A voxel of fewer than 3 points
// has eight zeros for a record: the callers' business.)  One eig3_sym.
__device__ __forceinline__ void wm_surfel(const MmlWmMoments& m, int np, float4& o0, float4& o1) {
    double c[6], ev[3], v2[3], v0[3];
    mml_wm_covariance(m, np, c);
    eig3_sym(c[0], c[1], c[2], c[3], c[4], c[5], ev, v2, v0);
    const double dot = (v0[0] * (double)m.vx + v0[1] * (double)m.vy) + v0[2] * (double)m.vz;
    if (dot < 0.0) {
        v0[0] = -v0[0];
        v0[1] = -v0[1];
        v0[2] = -v0[2];
    }
    double planarity = 0.0, linearity = 0.0;
    if (!(ev[2] <= 0.0)) {
        planarity = (ev[1] - ev[0]) / ev[2];
        linearity = (ev[2] - ev[1]) / ev[2];
    }
    o0 = make_float4((float)v0[0], (float)v0[1], (float)v0[2], (float)ev[0]);
    o1 = make_float4((float)ev[1], (float)ev[2], (float)planarity, (float)linearity);
}

// The surfel cache (mml_ctx::WorldMap::cache, read by k_wm_score): one float4 per table position, (nx, ny, nz, planarity) =
// o0.xyz, o1.z of wm_surfel for the position's moments and count; zeros below three points.
__device__ __forceinline__ float4 wm_cache_entry(const MmlWmMoments& m, int np) {
    if (np < 3) return make_float4(0.f, 0.f, 0.f, 0.f);
    float4 o0, o1;
    wm_surfel(m, np, o0, o1);
    return make_float4(o0.x, o0.y, o0.z, o1.z);
}

#endif
