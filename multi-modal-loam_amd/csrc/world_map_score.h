// world_map_score.h -- the one definition of the arithmetic of mml_world_map_score (world_map_score.hip): how well the surf stack
// of a slot fits a surfel map at a pose hypothesis.  Host and device, nothing of the project but world_map_assoc.h /
// world_map_key.h: a host program can include this file and check the arithmetic on its own
// (tests/cpp/world_map_score_check.cpp).  A feature goes through exactly the steps of mml_world_map_associate
// (world_map_assoc.h: world point, voxel, candidates, choice, the two gates); the table lookup and the winner's surfel are
// inputs, as there.  Everything that is summed is an integer, so a result does not depend on the order of the sum.
// One divide and one multiply in double beside the association's arithmetic, none contracted: built with -ffp-contract=off.
#ifndef MML_WORLD_MAP_SCORE_H
#define MML_WORLD_MAP_SCORE_H

#include "world_map_assoc.h"

#define MML_WMS_ONE 65536u  // the contribution of a match at |d| = 0

// what a feature is to a hypothesis
#define MML_WMS_SKIPPED 0    // mml_wma_voxel refused the world point: not counted at all
#define MML_WMS_NONE 1       // looked at: no candidate
#define MML_WMS_PLANARITY 2  // looked at: the winner's planarity is below the gate
#define MML_WMS_DISTANCE 3   // looked at: |d| is above the gate
#define MML_WMS_MATCH 4      // mml_world_map_associate would make a factor of it

// The features of a stack of n that a call with `stride` looks at: 0, stride, 2 stride, ... -- how many, and which one is the t-th.
MML_WM_HD int mml_wms_count(int n, int stride) { return n <= 0 ? 0 : (n - 1) / stride + 1; }
MML_WM_HD int mml_wms_feature(int t, int stride) { return t * stride; }

// The contribution of a match at plane distance d: 65536 at d = 0, 0 at |d| = max_plane_dist (> 0), truncated.  (A match has
// |d| <= max_plane_dist or a d that is not a number -- a surfel whose normal is not finite passes the gate's comparison, as in
// mml_wma_factor --; the latter contributes 0, so that the conversion is defined on both sides.)
MML_WM_HD unsigned mml_wms_quantum(double d, double max_plane_dist) {
    const double v = (1.0 - fabs(d) / max_plane_dist) * 65536.0;
    return v >= 0.0 ? (unsigned)v : 0u;
}

// One (slot, hypothesis): three integers.
struct MmlWmsAcc {
    unsigned long long score_q;
    int n_match, n_scored;
};
MML_WM_HD void mml_wms_init(MmlWmsAcc& a) {
    a.score_q = 0;
    a.n_match = a.n_scored = 0;
}
// A feature whose world point has a voxel (mml_wma_voxel held) against the choice `best` among its candidates (at < 0: none) and
// the winner's surfel (normal, planarity: read only when there is a winner).  Adds to the accumulator, returns the status.
MML_WM_HD int mml_wms_add(MmlWmsAcc& a, float wx, float wy, float wz, const MmlWmaBest& best, float nx, float ny, float nz, float planarity,
                          float min_planarity, double max_plane_dist) {
    a.n_scored += 1;
    if (best.at < 0) return MML_WMS_NONE;
    if (planarity < min_planarity) return MML_WMS_PLANARITY;
    double d = 0.0;
    if (!mml_wma_gates(wx, wy, wz, best.cx, best.cy, best.cz, nx, ny, nz, planarity, min_planarity, max_plane_dist, d)) return MML_WMS_DISTANCE;
    a.n_match += 1;
    a.score_q += mml_wms_quantum(d, max_plane_dist);
    return MML_WMS_MATCH;
}
// Ranking, wherever a best hypothesis is chosen: the larger score_q, then the larger n_match, then the smaller index.
MML_WM_HD bool mml_wms_better(unsigned long long qa, int ma, long ia, unsigned long long qb, int mb, long ib) {
    if (qa != qb) return qa > qb;
    if (ma != mb) return ma > mb;
    return ia < ib;
}

#endif
