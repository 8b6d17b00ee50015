// The arithmetic of csrc/voxel_sort_dev.h -- the order-preserving float key and pcl::VoxelGrid's index rules (MmlVoxGrid) -- checked
// on the host: built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_vox_grid.py and run as a process of its
// own.  The expected values are worked out here from PCL 1.8.1's rules (voxel_grid.hpp applyFilter) in plain integer / double code:
// a float product is the exact product of the two floats (it fits a double) rounded to float once.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define MML_VOXEL_ARITH_ONLY
#include "voxel_sort_dev.h"

static int fails = 0;
#define CHECK(cond)                                   \
    do {                                              \
        if (!(cond)) {                                \
            printf("line %d: %s\n", __LINE__, #cond); \
            ++fails;                                  \
        }                                             \
    } while (0)

static unsigned bits_of(float v) {
    unsigned u;
    memcpy(&u, &v, sizeof(u));
    return u;
}
static float float_of(unsigned u) {
    float v;
    memcpy(&v, &u, sizeof(v));
    return v;
}

// ---- the reference: PCL's rules without the header ---------------------------------------------------------------------------
static float ref_mul(float a, float b) { return (float)((double)a * (double)b); }
static long long ref_cell(float p, float inv) { return (long long)floor((double)ref_mul(p, inv)); }  // floor(p * inverse_leaf_size_)
struct RefGrid {
    long long min_b[3], div_b[3], voxels;
};
static RefGrid ref_grid(const float* mn, const float* mx, float inv) {
    RefGrid g;
    g.voxels = 1;
    for (int c = 0; c < 3; ++c) {
        g.min_b[c] = ref_cell(mn[c], inv);
        g.div_b[c] = ref_cell(mx[c], inv) - g.min_b[c] + 1;
        // the overflow rule counts with the truncated float extent: static_cast<int64_t>((max_p - min_p) * inverse_leaf_size_) + 1
        g.voxels *= (long long)ref_mul((float)((double)mx[c] - (double)mn[c]), inv) + 1;
    }
    return g;
}
static long long ref_index(const RefGrid& g, const float* p, float inv) {
    const long long i = ref_cell(p[0], inv) - g.min_b[0], j = ref_cell(p[1], inv) - g.min_b[1], k = ref_cell(p[2], inv) - g.min_b[2];
    return i + j * g.div_b[0] + k * g.div_b[0] * g.div_b[1];
}

// the box of `pts`, the header's grid against the reference's, every point's index against the reference's
static MmlVoxGrid check_cloud(const std::vector<float>& pts, float leaf) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < pts.size(); i += 3)
        for (int c = 0; c < 3; ++c) {
            mn[c] = fminf(mn[c], pts[i + c]);
            mx[c] = fmaxf(mx[c], pts[i + c]);
        }
    const MmlVoxGrid g = MmlVoxGrid::make(mn, mx, leaf);
    const float inv = 1.0f / leaf;
    const RefGrid r = ref_grid(mn, mx, inv);
    CHECK(bits_of(g.inv) == bits_of(inv));
    for (int c = 0; c < 3; ++c) CHECK(g.min_b[c] == r.min_b[c] && g.div_b[c] == r.div_b[c]);
    CHECK(g.overflows == (r.voxels > (long long)INT_MAX));
    // the same grid from the six keys the device kernels reduce the box into
    const int keys[6] = {mml_fkey(mn[0]), mml_fkey(mn[1]), mml_fkey(mn[2]), mml_fkey(mx[0]), mml_fkey(mx[1]), mml_fkey(mx[2])};
    const MmlVoxGrid k = mml_vox_grid_of_keys(keys, leaf);
    CHECK(memcmp(k.min_b, g.min_b, sizeof(g.min_b)) == 0 && memcmp(k.div_b, g.div_b, sizeof(g.div_b)) == 0 && k.overflows == g.overflows);
    if (!g.overflows)  // (an overflowing grid's index is never used: the callers key such a cloud by ordinal)
        for (size_t i = 0; i < pts.size(); i += 3) CHECK((long long)g.index(pts[i], pts[i + 1], pts[i + 2]) == ref_index(r, &pts[i], inv));
    return g;
}

int main() {
    // ---- the key ----
    const float denorm = float_of(1u);
    const float sorted[8] = {-INFINITY, -1.f, -denorm, -0.f, 0.f, denorm, 1.f, INFINITY};
    for (int i = 0; i < 8; ++i) {
        if (i) CHECK(mml_fkey(sorted[i - 1]) < mml_fkey(sorted[i]));  // strictly: -0.f below +0.f
        CHECK(bits_of(mml_funkey(mml_fkey(sorted[i]))) == bits_of(sorted[i]));
    }
    const float more[6] = {-3.4028235e38f, 3.4028235e38f, -0.05f, 1234.5678f, float_of(0x807fffffu), float_of(0x007fffffu)};
    for (float v : more) CHECK(bits_of(mml_funkey(mml_fkey(v))) == bits_of(v));
    const int empty[6] = MML_BBOX_EMPTY;
    for (int c = 0; c < 3; ++c) {
        CHECK(bits_of(mml_funkey(empty[c])) == bits_of(INFINITY));
        CHECK(bits_of(mml_funkey(empty[3 + c])) == bits_of(-INFINITY));
    }

    // ---- the grid ----
    {  // a single point
        const MmlVoxGrid g = check_cloud({1.0f, -2.0f, 3.5f}, 0.5f);
        CHECK(g.div_b[0] == 1 && g.div_b[1] == 1 && g.div_b[2] == 1 && !g.overflows);
        CHECK(g.min_b[0] == 2 && g.min_b[1] == -4 && g.min_b[2] == 7);
        CHECK(g.index(1.0f, -2.0f, 3.5f) == 0u);
    }
    {  // either side of a voxel face at negative coordinates: 1 / 0.05f is 20.f; -0.05f * 20.f rounds to -1.f, one ulp towards zero
       // gives -(1 - 2^-24), both cell -1; one ulp away gives -(1 + 2^-23), cell -2
        const float face = -0.05f, inner = nextafterf(face, 0.f), outer = nextafterf(face, -1.f);
        const MmlVoxGrid g = check_cloud({inner, 0.f, 0.f, outer, 0.f, 0.f, face, 0.f, 0.f}, 0.05f);
        CHECK(bits_of(g.inv) == bits_of(20.f));
        CHECK(g.min_b[0] == -2 && g.div_b[0] == 2 && g.div_b[1] == 1 && g.div_b[2] == 1);
        CHECK(g.index(outer, 0.f, 0.f) == 0u && g.index(face, 0.f, 0.f) == 1u && g.index(inner, 0.f, 0.f) == 1u);
    }
    {  // The int32 rule, "more than INT_MAX voxels", flips between 2^31 - 2 and 2^31: INT_MAX itself is prime, so a box of exactly
       // INT_MAX voxels would need all of them along one axis, an extent float coordinates cannot express (floats that large are
       // multiples of 128).  2^31 - 2 = 1386 * 4681 * 331 is the largest count at or below INT_MAX a box can have.
        const MmlVoxGrid below = check_cloud({0.f, 0.f, 0.f, 1385.f, 4680.f, 330.f}, 1.0f);
        CHECK(!below.overflows && (long long)below.div_b[0] * below.div_b[1] * below.div_b[2] == (long long)INT_MAX - 1);
        CHECK(below.index(1385.f, 4680.f, 330.f) == (unsigned)(INT_MAX - 2));  // the last voxel's index still fits an int
        const MmlVoxGrid one_more = check_cloud({0.f, 0.f, 0.f, 1386.f, 4680.f, 330.f}, 1.0f);  // one voxel more along x
        CHECK(one_more.overflows);
        const MmlVoxGrid above = check_cloud({0.f, 0.f, 0.f, 2047.f, 1023.f, 1023.f}, 1.0f);  // 2^31 voxels: the first count above
        CHECK(above.overflows && (long long)above.div_b[0] * above.div_b[1] * above.div_b[2] == (long long)INT_MAX + 1);
    }
    {  // max == min, three times the same point
        const MmlVoxGrid g = check_cloud({-3.3f, 7.7f, -0.f, -3.3f, 7.7f, -0.f, -3.3f, 7.7f, -0.f}, 0.4f);
        CHECK(g.div_b[0] == 1 && g.div_b[1] == 1 && g.div_b[2] == 1 && !g.overflows && g.index(-3.3f, 7.7f, -0.f) == 0u);
    }
    for (float leaf : {0.4f, 0.05f, 0.2f}) {  // a scattered cloud around the origin
        std::vector<float> pts;
        unsigned lcg = 12345u;
        for (int i = 0; i < 3000; ++i) {
            lcg = lcg * 1664525u + 1013904223u;
            pts.push_back(((int)(lcg >> 8) % 2000001 - 1000000) * 1e-5f);  // [-10, 10]
        }
        check_cloud(pts, leaf);
    }
    if (fails == 0) printf("vox_grid_check ok\n");
    return fails ? 1 : 0;
}
