// world_map_evict.h -- the one definition of which voxels mml_world_map_evict removes (world_map.hip k_wm_evict_mark, and the host
// check tests/cpp/world_map_evict_check.cpp): the rule of one map, the decision for one voxel and the conversion of a metric box
// into voxel indices.  Host and device, no other header of the project needed but world_map_key.h.  The decision compares
// integers only: a box is given in voxel indices, so that no float comparison takes part in it.
#ifndef MML_WORLD_MAP_EVICT_H
#define MML_WORLD_MAP_EVICT_H

#include "world_map_key.h"

// (include/mmloam_hip.h declares the same rule under the same guard)
#ifndef MML_WM_EVICT_RULE_DEFINED
#define MML_WM_EVICT_RULE_DEFINED
#define MML_WM_EVICT_OUTSIDE 0   /* voxels outside the box go */
#define MML_WM_EVICT_INSIDE  1   /* voxels inside the box go  */
#define MML_WM_EVICT_NOBOX   2   /* the box is not read; only min_count decides */
typedef struct {
    int map;            /* 0 .. n_maps-1; a map may be named by at most one rule of a call */
    int mode;
    int lo[3], hi[3];   /* voxel indices i, j, k: inside means lo[a] <= index[a] < hi[a] on all three axes */
    int min_count;      /* a voxel whose point count is < min_count goes as well; 0 or 1: none does */
} mml_wm_evict_rule;
#endif

// inside the box: lo[a] <= index[a] < hi[a] on all three axes; a box with lo[a] >= hi[a] on some axis holds nothing
MML_WM_HD bool mml_wme_inside(const mml_wm_evict_rule& r, int i, int j, int k) {
    return i >= r.lo[0] && i < r.hi[0] && j >= r.lo[1] && j < r.hi[1] && k >= r.lo[2] && k < r.hi[2];
}
// The whole decision for voxel (i, j, k) of the rule's map holding `count` points: the box test by mode, OR the count test.  An
// empty box evicts the map under OUTSIDE and nothing under INSIDE.  A stored count is >= 1, so min_count 0 and 1 evict nothing
// and a caller that knows min_count <= 1 may pass any count >= 1.
MML_WM_HD bool mml_wme_goes(const mml_wm_evict_rule& r, int i, int j, int k, int count) {
    bool box = false;
    if (r.mode == MML_WM_EVICT_OUTSIDE) box = !mml_wme_inside(r, i, j, k);
    if (r.mode == MML_WM_EVICT_INSIDE) box = mml_wme_inside(r, i, j, k);
    return box || count < r.min_count;
}

// One coordinate of a metric box as a voxel index: mml_wm_axis's arithmetic (the product in float, floor of its double), plus
// `plus`, clamped to [-2^17, 2^17] -- a product that overflowed included.
MML_WM_HD int mml_wme_index(float v, float inv, int plus) {
    double f = floor((double)(v * inv)) + (double)plus;
    if (!(f >= -(double)MML_WM_HALF)) f = -(double)MML_WM_HALF;  // (v and inv are finite: the product is no NaN)
    if (f > (double)MML_WM_HALF) f = (double)MML_WM_HALF;
    return (int)f;
}
// The index box of the metric box [lo_xyz, hi_xyz] of a map of leaf size `leaf`: lo = index(lo_xyz), hi = index(hi_xyz) + 1, so
// that the voxel a corner lies in is inside.  0, or -1 (nothing written) when the leaf is not finite and positive or a coordinate
// is not finite.
MML_WM_HD int mml_wme_index_box(float leaf, const float lo_xyz[3], const float hi_xyz[3], int lo[3], int hi[3]) {
    if (!mml_wm_finite(leaf) || !(leaf > 0.f)) return -1;
    for (int a = 0; a < 3; ++a)
        if (!mml_wm_finite(lo_xyz[a]) || !mml_wm_finite(hi_xyz[a])) return -1;
    const float inv = mml_wm_inv_leaf(leaf);
    for (int a = 0; a < 3; ++a) {
        lo[a] = mml_wme_index(lo_xyz[a], inv, 0);
        hi[a] = mml_wme_index(hi_xyz[a], inv, 1);
    }
    return 0;
}

#endif
