// world_map_dev.h -- what the world map's kernels in more than one translation unit share (world_map.hip, world_map_assoc.hip):
// the per-wave counter add, the read-only probe, the moment arrays and the surfel record of one voxel.  Device only; include
// inside an anonymous namespace of the translation unit, behind eig3_dev.h.
#ifndef MML_WORLD_MAP_DEV_H
#define MML_WORLD_MAP_DEV_H

#include "world_map_key.h"

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

// the three moment arrays of a surfel map (or of a reset's scratch copy); null in a plain map
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

#endif
