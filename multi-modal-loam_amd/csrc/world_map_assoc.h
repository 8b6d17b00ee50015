// world_map_assoc.h -- the one definition of the arithmetic of mml_world_map_associate (world_map_assoc.hip): which voxels a
// feature is matched against, which of them wins, the gates on the winner's surfel and the plane factor it yields.  Host and
// device, nothing of the project but world_map_key.h: a host program can include this file and check the arithmetic on its own
// (tests/cpp/world_map_assoc_check.cpp).  What is NOT here: the table lookup (wm_find) and the surfel record of the winner
// (wm_surfel: the eigen-solver is device only) -- both are inputs of the functions below.
// Adds, multiplies, divides and one square root, none contracted: built with -ffp-contract=off like world_map_key.h.
#ifndef MML_WORLD_MAP_ASSOC_H
#define MML_WORLD_MAP_ASSOC_H

#include "world_map_key.h"

// The voxel (i, j, k) of the float world point w; false (the feature is skipped) when a coordinate is not finite or an index
// leaves [-2^17, 2^17).
MML_WM_HD bool mml_wma_voxel(float wx, float wy, float wz, float inv, int& i, int& j, int& k) {
    if (!(mml_wm_finite(wx) && mml_wm_finite(wy) && mml_wm_finite(wz))) return false;
    return mml_wm_axis(wx, inv, i) && mml_wm_axis(wy, inv, j) && mml_wm_axis(wz, inv, k);
}
// Candidate (i, j, k) of map `map`: false when an index lies outside the range or the packed key is the free marker (a lookup of
// the marker would "find" the first free position), else true with the key.
MML_WM_HD bool mml_wma_candidate(int map, int i, int j, int k, unsigned long long& key) {
    if (i < -MML_WM_HALF || i >= MML_WM_HALF || j < -MML_WM_HALF || j >= MML_WM_HALF || k < -MML_WM_HALF || k >= MML_WM_HALF) return false;
    key = mml_wm_key(map, i, j, k);
    return key != MML_WM_EMPTY;
}
// the squared distance of w to a candidate's centroid c = sum.xyz / (float)count (mml_wm_centroid): differences and products in
// double from the float values
MML_WM_HD double mml_wma_r2(float wx, float wy, float wz, float cx, float cy, float cz) {
    const double dx = (double)wx - (double)cx, dy = (double)wy - (double)cy, dz = (double)wz - (double)cz;
    return (dx * dx + dy * dy) + dz * dz;
}
// The choice among the candidates: the smallest r2, ties to the smaller packed key.  `at` is whatever the caller needs to find
// the winner again (the table position), n its point count; at < 0: no candidate yet.
struct MmlWmaBest {
    double r2;
    unsigned long long key;
    long long at;
    int n;
    float cx, cy, cz;
};
MML_WM_HD void mml_wma_best_init(MmlWmaBest& b) {
    b.r2 = 0.0;
    b.key = 0;
    b.at = -1;
    b.n = 0;
    b.cx = b.cy = b.cz = 0.f;
}
MML_WM_HD void mml_wma_offer(MmlWmaBest& b, double r2, unsigned long long key, long long at, int n, float cx, float cy, float cz) {
    if (b.at < 0 || r2 < b.r2 || (r2 == b.r2 && key < b.key)) {
        b.r2 = r2;
        b.key = key;
        b.at = at;
        b.n = n;
        b.cx = cx;
        b.cy = cy;
        b.cz = cz;
    }
}
// The plane factor of feature f (world point w, pose T row-major) against the winner: centroid c, surfel normal n and planarity
// as the surfel record holds them.  Returns 1 with the record, 0 when a gate rejects the winner (there is no second choice).
struct MmlWmaFactor {
    float ori[3];
    float omega[3];
    double proj[3];
    double error;
};
// the signed distance of w to the plane through the centroid c with the normal n: differences and products in double
MML_WM_HD double mml_wma_plane_dist(float wx, float wy, float wz, float cx, float cy, float cz, float nx, float ny, float nz) {
    return ((double)nx * ((double)wx - (double)cx) + (double)ny * ((double)wy - (double)cy)) + (double)nz * ((double)wz - (double)cz);
}
// The two gates on the winner, and the distance they leave: false when the planarity or |d| rejects it.  mml_wma_factor and the
// pose score (world_map_score.h) both decide through this function.
MML_WM_HD bool mml_wma_gates(float wx, float wy, float wz, float cx, float cy, float cz, float nx, float ny, float nz, float planarity,
                             float min_planarity, double max_plane_dist, double& d) {
    if (planarity < min_planarity) return false;
    d = mml_wma_plane_dist(wx, wy, wz, cx, cy, cz, nx, ny, nz);
    return !(fabs(d) > max_plane_dist);
}
MML_WM_HD int mml_wma_factor(const double* T, float fx, float fy, float fz, float wx, float wy, float wz, float cx, float cy, float cz,
                             float nx, float ny, float nz, float planarity, float min_planarity, double max_plane_dist, MmlWmaFactor& out) {
    double d = 0.0;
    if (!mml_wma_gates(wx, wy, wz, cx, cy, cz, nx, ny, nz, planarity, min_planarity, max_plane_dist, d)) return 0;
    out.ori[0] = fx;
    out.ori[1] = fy;
    out.ori[2] = fz;
    out.omega[0] = nx;
    out.omega[1] = ny;
    out.omega[2] = nz;
    out.proj[0] = (double)wx - d * (double)nx;
    out.proj[1] = (double)wy - d * (double)ny;
    out.proj[2] = (double)wz - d * (double)nz;
    // the error of a plane factor (Estimator.h:118-121): the double transform of f, not the float world point
    const double x = (double)fx, y = (double)fy, z = (double)fz;
    const double px = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    const double py = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    const double pz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    const double ex = px - out.proj[0], ey = py - out.proj[1], ez = pz - out.proj[2];
    out.error = sqrt((ex * ex + ey * ey) + ez * ez);
    return 1;
}

#endif
