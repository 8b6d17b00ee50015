// world_map_key.h -- the one definition of the world map's arithmetic (world_map.hip, mml_world_map_*): the world point, the voxel
// index, the 64-bit key, the hash of a key to a table position, the per-voxel accumulator and, for a surfel map, the per-voxel
// moments and the covariance they give (the eigen-decomposition of it is eig3_dev.h's, device only).  Host and device, no other header
// of the project needed: a host program can include this file and check the arithmetic on its own
// (tests/cpp/world_map_key_check.cpp), or compute which keys collide in a table of a given size.
// Adds, multiplies and divides only, none of them contracted: every translation unit that includes this file is built with
// -ffp-contract=off (the Makefile's FLAGS; the host check passes it too).
#ifndef MML_WORLD_MAP_KEY_H
#define MML_WORLD_MAP_KEY_H

#include <math.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MML_WM_HD __host__ __device__ __forceinline__
#else
#define MML_WM_HD inline
#endif

#define MML_WM_AXIS_BITS 18                       // bits of one axis inside a key
#define MML_WM_HALF (1 << (MML_WM_AXIS_BITS - 1)) // voxel indices lie in [-2^17, 2^17)
#define MML_WM_MAP_SHIFT (3 * MML_WM_AXIS_BITS)   // 54: the map number sits above the three axes
#define MML_WM_MAPS_MAX 1024                      // = MML_MAP_BANKS_MAX: 10 bits
#define MML_WM_EMPTY (~0ull)                      // the marker of a free table position
// what mml_wm_classify says of a point
#define MML_WM_KEPT 0
#define MML_WM_NONFINITE 1
#define MML_WM_OUT_OF_RANGE 2

// pointAssociateToMap (unionPoseEstimation.cpp:199-213), the world point of every registered cloud: pout = R * pin + t in double,
// in Eigen's order (R0 x + R1 y) + R2 z, then + t, no contraction, rounded once to float.  T: a row-major 4 x 4 pose, of which
// the upper three rows are applied as given.  k_encode_registered (mml_cloud_download_registered_batch) and the world map's key
// kernel both go through this function.
MML_WM_HD void mml_world_point(const double* T, double x, double y, double z, float& ox, float& oy, float& oz) {
    ox = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
    oy = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
    oz = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
}

MML_WM_HD bool mml_wm_finite(float v) {
    unsigned b;
    __builtin_memcpy(&b, &v, sizeof(b));
    return (b & 0x7f800000u) != 0x7f800000u;
}
// the inverse leaf, a float (MmlVoxGrid's inverse_leaf_size_)
MML_WM_HD float mml_wm_inv_leaf(float leaf) { return 1.0f / leaf; }
// One axis: floor (the double overload) of the float product, MmlVoxGrid's convention.  Returns false when the index lies outside
// [-2^17, 2^17) -- a product that overflowed to infinity included --, else true with the index in i.
MML_WM_HD bool mml_wm_axis(float v, float inv, int& i) {
    const double f = floor((double)(v * inv));
    if (!(f >= -(double)MML_WM_HALF && f < (double)MML_WM_HALF)) return false;
    i = (int)f;
    return true;
}
// map << 54 | (k + 2^17) << 36 | (j + 2^17) << 18 | (i + 2^17)
MML_WM_HD unsigned long long mml_wm_key(int map, int i, int j, int k) {
    return ((unsigned long long)map << MML_WM_MAP_SHIFT) | ((unsigned long long)(k + MML_WM_HALF) << (2 * MML_WM_AXIS_BITS)) |
           ((unsigned long long)(j + MML_WM_HALF) << MML_WM_AXIS_BITS) | (unsigned long long)(i + MML_WM_HALF);
}
MML_WM_HD void mml_wm_unkey(unsigned long long key, int& map, int& i, int& j, int& k) {
    const unsigned long long m = (1ull << MML_WM_AXIS_BITS) - 1;
    map = (int)(key >> MML_WM_MAP_SHIFT);
    k = (int)((key >> (2 * MML_WM_AXIS_BITS)) & m) - MML_WM_HALF;
    j = (int)((key >> MML_WM_AXIS_BITS) & m) - MML_WM_HALF;
    i = (int)(key & m) - MML_WM_HALF;
}
// A world point (x, y, z, intensity) of map `map` (0 .. 1023): MML_WM_NONFINITE when a coordinate or the intensity is not finite,
// MML_WM_OUT_OF_RANGE when an index leaves [-2^17, 2^17), else MML_WM_KEPT with its key.  The 64 bits are all in use, so ONE
// packed key equals the empty marker: map 1023, voxel (2^17 - 1, 2^17 - 1, 2^17 - 1).  That voxel of that map counts as out of
// range, so that no kept point ever carries the marker.
MML_WM_HD int mml_wm_classify(int map, float x, float y, float z, float w, float inv, unsigned long long& key) {
    if (!(mml_wm_finite(x) && mml_wm_finite(y) && mml_wm_finite(z) && mml_wm_finite(w))) return MML_WM_NONFINITE;
    int i, j, k;
    if (!(mml_wm_axis(x, inv, i) && mml_wm_axis(y, inv, j) && mml_wm_axis(z, inv, k))) return MML_WM_OUT_OF_RANGE;
    key = mml_wm_key(map, i, j, k);
    return key == MML_WM_EMPTY ? MML_WM_OUT_OF_RANGE : MML_WM_KEPT;
}

// The first position a key is tried at in a table of `slots` positions (a power of two, at least 2): the 64-bit finaliser of
// splitmix64, masked.  A key that finds its position taken goes on to (position + 1) & (slots - 1), and so on.
MML_WM_HD unsigned long long mml_wm_hash(unsigned long long key, unsigned long long slots) {
    key ^= key >> 30;
    key *= 0xbf58476d1ce4e5b9ull;
    key ^= key >> 27;
    key *= 0x94d049bb133111ebull;
    key ^= key >> 31;
    return key & (slots - 1);
}
// the table of a map of `capacity_voxels`: the next power of two >= 2 x capacity
MML_WM_HD unsigned long long mml_wm_table_slots(long long capacity_voxels) {
    unsigned long long s = 2;
    while (s < 2ull * (unsigned long long)capacity_voxels) s <<= 1;
    return s;
}

// One voxel: the float sums of x, y, z, intensity and the point count.  Points are added one after the other, starting from the
// stored sum; the centroid is sum / (float)count per field.
struct MmlWmAcc {
    float x, y, z, w;
    int n;
};
MML_WM_HD void mml_wm_add(MmlWmAcc& a, float x, float y, float z, float w) {
    a.x += x;
    a.y += y;
    a.z += z;
    a.w += w;
    a.n += 1;
}
MML_WM_HD void mml_wm_centroid(const MmlWmAcc& a, float out[4]) {
    const float c = (float)a.n;
    out[0] = a.x / c;
    out[1] = a.y / c;
    out[2] = a.z / c;
    out[3] = a.w / c;
}

// ---- surfel maps (MML_WM_SURFELS): the second moments of a voxel's points about the voxel's centre, and their view sum ----
// the centre of voxel index i (what mml_wm_axis returned) on one axis: (float)i + 0.5f is exact for |i| <= 2^17, one rounding
MML_WM_HD float mml_wm_centre(int i, float leaf) { return ((float)i + 0.5f) * leaf; }
// the sensor origin of a slot: the translation of its row-major pose, each rounded to float
MML_WM_HD void mml_wm_origin(const double* T, float& ox, float& oy, float& oz) {
    ox = (float)T[3];
    oy = (float)T[7];
    oz = (float)T[11];
}
// One voxel, 12 floats as three float4 of the table: the sums of the offsets d = w - centre, of their six products and of the
// view vectors v = origin - w.
struct MmlWmMoments {
    float sdx, sdy, sdz, vx;
    float sxx, sxy, sxz, vy;
    float syy, syz, szz, vz;
};
// One world point (wx, wy, wz) of the voxel centred at (cx, cy, cz), seen from (ox, oy, oz): every difference and every product
// is rounded to float on its own and then added, in the order written.
MML_WM_HD void mml_wm_add_moments(MmlWmMoments& m, float wx, float wy, float wz, float cx, float cy, float cz, float ox, float oy,
                                  float oz) {
    const float dx = wx - cx, dy = wy - cy, dz = wz - cz;
    m.sdx += dx;
    m.sdy += dy;
    m.sdz += dz;
    const float xx = dx * dx, xy = dx * dy, xz = dx * dz, yy = dy * dy, yz = dy * dz, zz = dz * dz;
    m.sxx += xx;
    m.sxy += xy;
    m.sxz += xz;
    m.syy += yy;
    m.syz += yz;
    m.szz += zz;
    const float px = ox - wx, py = oy - wy, pz = oz - wz;
    m.vx += px;
    m.vy += py;
    m.vz += pz;
}
// The covariance of a voxel of n points about its mean, in double, as the lower triangle the eigen-solver takes:
// c = {Cxx, Cxy, Cyy, Cxz, Cyz, Czz} = m00 m10 m11 m20 m21 m22, C_ab = s_ab / n - m_a m_b with m_a = sd_a / n.
MML_WM_HD void mml_wm_covariance(const MmlWmMoments& m, int n, double c[6]) {
    const double nd = (double)n;
    const double mx = (double)m.sdx / nd, my = (double)m.sdy / nd, mz = (double)m.sdz / nd;
    c[0] = (double)m.sxx / nd - mx * mx;
    c[1] = (double)m.sxy / nd - mx * my;
    c[2] = (double)m.syy / nd - my * my;
    c[3] = (double)m.sxz / nd - mx * mz;
    c[4] = (double)m.syz / nd - my * mz;
    c[5] = (double)m.szz / nd - mz * mz;
}

#endif
