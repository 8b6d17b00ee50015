// fused_view_dev.h -- the fused cloud of a slot as the kernels at the API boundary read it: FusedView / fused_at (one slot),
// SlotArrays / slot_view (a kernel over the slots [first, ...) derives the view on the device) and slot_arrays, the host side of
// the latter.  Shared by capi.hip (the downloads) and world_map.hip (the world map's key kernel).  Needs mml_internal.h first.
#ifndef MML_FUSED_VIEW_DEV_H
#define MML_FUSED_VIEW_DEV_H

// The fused cloud [velo_combine ; livox_combine] in its own order, gathered from the line-bucketed storage: position pos
// (Velodyne region [0, cv), Livox region [NV, NV + cl)) holds fused point ln_gidx[pos] when that is >= 0.  The Velodyne
// part of an extracted cloud carries intensity 0 (unionFeatureExtract.cpp:1254-1256); an uploaded cloud keeps its own.
struct FusedView {
    const float4* pts;
    const int* gidx;
    const int* rel;
    const uint8_t* line;      // uploaded clouds
    const uint8_t* label;
    const int* cb_n;          // this slot's two valid counts
    const int* seg_flat;      // extracted clouds: per sensor the starts of the storage segments in storage order (block-major,
    const int* seg_flat_n;    //   line inside a block) -- 2 x MML_SEG_FLAT ints -- and (entries, lines per block) per sensor
    int NV, NT, L, n_rings, flags;
};
__device__ __forceinline__ bool fused_at(const FusedView& V, int pos, int& g, float4& p, float& rel, int& line) {
    if (pos >= V.NT) return false;
    if (pos < V.NV ? pos >= V.cb_n[0] : pos - V.NV >= V.cb_n[1]) return false;
    g = V.gidx[pos];
    if (g < 0) return false;
    p = V.pts[pos];
    rel = (V.flags & 2) ? 1.0f : __int_as_float(V.rel[pos]);  // RemoveLidarDistortion leaves normal_x = 1 (unionPoseEstimation.cpp:419)
    if (V.flags & 1) {
        line = V.line[pos];
    } else {
        if (pos < V.NV) p.w = 0.f;  // intensity of the Velodyne part is zeroed (unionFeatureExtract.cpp:1254-1256)
        // last storage segment of the region whose start is <= pos (starts are non-decreasing; an empty segment shares its start
        // with the next one); segment f belongs to line f mod (lines per block)
        const int sensor = pos < V.NV ? 0 : 1;
        const int* flat = V.seg_flat + sensor * MML_SEG_FLAT;
        int lo = 0, hi = V.seg_flat_n[2 * sensor] - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (flat[mid] <= pos)
                lo = mid;
            else
                hi = mid - 1;
        }
        line = lo % V.seg_flat_n[2 * sensor + 1];
    }
    return true;
}
// the per-point and per-slot arrays of a context that a kernel over the slots [first, ...) indexes by slot
struct SlotArrays {
    const float4* pts;
    const int* gidx;
    const int* rel;
    const uint8_t* line;
    const uint8_t* label;
    const int* cb_n;
    const int* seg_flat;
    const int* seg_flat_n;
    const int* slot_flags;
    const int* fu_info;
    int NV, NT, L, n_rings, first;
};
// The FusedView of one slot, derived on the device from the context-wide arrays; the flag word is read here, where fused_view
// spends a synchronising read-back per slot.
__device__ __forceinline__ FusedView slot_view(const SlotArrays& A, int slot) {
    FusedView V;
    const size_t off = (size_t)slot * A.NT;
    V.pts = A.pts + off;
    V.gidx = A.gidx + off;
    V.rel = A.rel + off;
    V.line = A.line + off;
    V.label = A.label + off;
    V.cb_n = A.cb_n + 2 * (size_t)slot;
    V.seg_flat = A.seg_flat + (size_t)slot * 2 * MML_SEG_FLAT;
    V.seg_flat_n = A.seg_flat_n + (size_t)slot * 4;
    V.NV = A.NV;
    V.NT = A.NT;
    V.L = A.L;
    V.n_rings = A.n_rings;
    V.flags = A.slot_flags[2 * (size_t)slot];
    return V;
}
inline SlotArrays slot_arrays(const mml_ctx* ctx, int first) {
    SlotArrays A;
    A.pts = ctx->ln_pts;
    A.gidx = ctx->ln_gidx;
    A.rel = ctx->ln_rel;
    A.line = ctx->ln_line;
    A.label = ctx->ln_label;
    A.cb_n = ctx->cb_n;
    A.seg_flat = ctx->seg_flat;
    A.seg_flat_n = ctx->seg_flat_n;
    A.slot_flags = ctx->slot_flags;
    A.fu_info = ctx->fu_info;
    A.NV = ctx->NV;
    A.NT = ctx->NT;
    A.L = ctx->L;
    A.n_rings = ctx->cfg.n_rings;
    A.first = first;
    return A;
}

#endif
