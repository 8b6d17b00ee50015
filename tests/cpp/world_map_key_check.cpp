// Stand-alone host check of csrc/world_map_key.h (the world map's arithmetic); includes nothing else of the project.
// Prints "world_map_key_check ok" and returns 0, or says what failed and returns 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>

#include "world_map_key.h"

static int fails = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("line %d: %s\n", __LINE__, #cond);                \
            ++fails;                                                 \
        }                                                            \
    } while (0)

static float below(float v) { return nextafterf(v, -std::numeric_limits<float>::infinity()); }

int main() {
    const float leaf = 0.25f, inv = mml_wm_inv_leaf(leaf);  // a power of two: v * inv is exact, the expected indices are plain
    CHECK(inv == 4.0f);
    int i = 99;
    // floor, not truncation
    CHECK(mml_wm_axis(-0.f, inv, i) && i == 0);
    CHECK(mml_wm_axis(0.f, inv, i) && i == 0);
    CHECK(mml_wm_axis(-leaf, inv, i) && i == -1);           // -leaf exactly: the voxel [-leaf, 0)
    CHECK(mml_wm_axis(below(0.f), inv, i) && i == -1);      // the float just below 0 (a denormal)
    CHECK(mml_wm_axis(below(-leaf), inv, i) && i == -2);
    CHECK(mml_wm_axis(below(leaf), inv, i) && i == 0);
    CHECK(mml_wm_axis(leaf, inv, i) && i == 1);
    // +-(2^17 - 1) voxels, and the first index out of range on both sides
    const float hi = (float)(MML_WM_HALF - 1) * leaf, lo = -(float)(MML_WM_HALF - 1) * leaf;
    CHECK(mml_wm_axis(hi, inv, i) && i == MML_WM_HALF - 1);
    CHECK(mml_wm_axis(below((float)MML_WM_HALF * leaf), inv, i) && i == MML_WM_HALF - 1);
    CHECK(!mml_wm_axis((float)MML_WM_HALF * leaf, inv, i));                 // index 2^17: the first outside above
    CHECK(mml_wm_axis(lo, inv, i) && i == -(MML_WM_HALF - 1));
    CHECK(mml_wm_axis(-(float)MML_WM_HALF * leaf, inv, i) && i == -MML_WM_HALF);  // index -2^17: the last inside below
    CHECK(!mml_wm_axis(below(-(float)MML_WM_HALF * leaf), inv, i));         // index -2^17 - 1: the first outside below
    CHECK(!mml_wm_axis(3.0e38f, inv, i));                                   // the product overflows to infinity
    CHECK(!mml_wm_axis(-3.0e38f, inv, i));
    CHECK(!mml_wm_axis(1.0e30f, inv, i));                                   // beyond int: refused before any conversion
    // a leaf that is no power of two: the index is floor of the FLOAT product
    {
        const float l2 = 0.2f, inv2 = mml_wm_inv_leaf(l2), v = 0.6f;
        const float prod = v * inv2;
        CHECK(mml_wm_axis(v, inv2, i) && i == (int)floor((double)prod));
    }
    // classification
    unsigned long long key = 0;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(mml_wm_classify(0, 0.f, 0.f, 0.f, 1.f, inv, key) == MML_WM_KEPT && key == mml_wm_key(0, 0, 0, 0));
    CHECK(mml_wm_classify(0, nan, 0.f, 0.f, 1.f, inv, key) == MML_WM_NONFINITE);
    CHECK(mml_wm_classify(0, 0.f, inf, 0.f, 1.f, inv, key) == MML_WM_NONFINITE);
    CHECK(mml_wm_classify(0, 0.f, 0.f, -inf, 1.f, inv, key) == MML_WM_NONFINITE);
    CHECK(mml_wm_classify(0, 0.f, 0.f, 0.f, nan, inv, key) == MML_WM_NONFINITE);
    CHECK(mml_wm_classify(0, nan, 1.0e30f, 0.f, 1.f, inv, key) == MML_WM_NONFINITE);  // (not finite comes first)
    CHECK(mml_wm_classify(0, 1.0e30f, 0.f, 0.f, 1.f, inv, key) == MML_WM_OUT_OF_RANGE);
    // key packing round-trip at the corners, and key 0 is reachable
    const int edge[4] = {-MML_WM_HALF, -1, 0, MML_WM_HALF - 1};
    const int maps[4] = {0, 1, 511, MML_WM_MAPS_MAX - 1};
    for (int m : maps)
        for (int a : edge)
            for (int b : edge)
                for (int c : edge) {
                    const unsigned long long k = mml_wm_key(m, a, b, c);
                    int m2, a2, b2, c2;
                    mml_wm_unkey(k, m2, a2, b2, c2);
                    CHECK(m2 == m && a2 == a && b2 == b && c2 == c);
                }
    CHECK(mml_wm_key(0, -MML_WM_HALF, -MML_WM_HALF, -MML_WM_HALF) == 0ull);
    CHECK(mml_wm_key(0, 1 - MML_WM_HALF, -MML_WM_HALF, -MML_WM_HALF) == 1ull);
    CHECK(mml_wm_key(0, -MML_WM_HALF, 1 - MML_WM_HALF, -MML_WM_HALF) == 1ull << 18);
    CHECK(mml_wm_key(0, -MML_WM_HALF, -MML_WM_HALF, 1 - MML_WM_HALF) == 1ull << 36);
    CHECK(mml_wm_key(1, -MML_WM_HALF, -MML_WM_HALF, -MML_WM_HALF) == 1ull << 54);
    // the empty marker is never the key of a kept point: all 64 bits are in use, the one packed key that equals it is refused
    CHECK(mml_wm_key(MML_WM_MAPS_MAX - 1, MML_WM_HALF - 1, MML_WM_HALF - 1, MML_WM_HALF - 1) == MML_WM_EMPTY);
    CHECK(mml_wm_classify(MML_WM_MAPS_MAX - 1, hi, hi, hi, 1.f, inv, key) == MML_WM_OUT_OF_RANGE);
    CHECK(mml_wm_classify(MML_WM_MAPS_MAX - 1, hi, hi, hi - leaf, 1.f, inv, key) == MML_WM_KEPT && key != MML_WM_EMPTY);
    CHECK(mml_wm_classify(MML_WM_MAPS_MAX - 2, hi, hi, hi, 1.f, inv, key) == MML_WM_KEPT && key != MML_WM_EMPTY);
    for (int m : maps)
        for (int a : edge)
            for (int b : edge)
                for (int c : edge) {
                    const int what = mml_wm_classify(m, a * leaf, b * leaf, c * leaf, 0.f, inv, key);
                    CHECK(what == MML_WM_OUT_OF_RANGE || (what == MML_WM_KEPT && key != MML_WM_EMPTY && key == mml_wm_key(m, a, b, c)));
                }
    // the hash stays inside the table, for 2 positions and for 2^20, and reaches both ends of the small one
    CHECK(mml_wm_table_slots(1) == 2 && mml_wm_table_slots(2) == 4 && mml_wm_table_slots(3) == 8 && mml_wm_table_slots(4) == 8 &&
          mml_wm_table_slots(64) == 128 && mml_wm_table_slots(1 << 19) == 1 << 20);
    int seen[2] = {0, 0};
    unsigned long long k = 0x9e3779b97f4a7c15ull;
    for (int r = 0; r < 100000; ++r) {
        k = k * 6364136223846793005ull + 1442695040888963407ull;
        const unsigned long long h2 = mml_wm_hash(k, 2), h20 = mml_wm_hash(k, 1ull << 20);
        CHECK(h2 < 2 && h20 < (1ull << 20));
        ++seen[h2 & 1];
    }
    CHECK(seen[0] > 0 && seen[1] > 0);
    CHECK(mml_wm_hash(0, 2) < 2 && mml_wm_hash(MML_WM_EMPTY - 1, 2) < 2 && mml_wm_hash(MML_WM_EMPTY - 1, 1ull << 20) < (1ull << 20));
    // the accumulator: float adds in the order given (the two orders of three values differ), one float divide
    {
        const float a = 1.0e8f, b = -1.0e8f, c = 1.0f;
        MmlWmAcc p = {0.f, 0.f, 0.f, 0.f, 0}, q = p;
        mml_wm_add(p, a, a, a, a);
        mml_wm_add(p, b, b, b, b);
        mml_wm_add(p, c, c, c, c);
        mml_wm_add(q, a, a, a, a);
        mml_wm_add(q, c, c, c, c);
        mml_wm_add(q, b, b, b, b);
        CHECK(p.n == 3 && q.n == 3 && p.x == 1.0f && q.x == 0.0f && p.w == 1.0f && q.w == 0.0f);
        float cen[4];
        mml_wm_centroid(p, cen);
        CHECK(cen[0] == 1.0f / 3.0f && cen[3] == 1.0f / 3.0f);
    }
    // the world point: double, (R0 x + R1 y) + R2 z, then + t, one rounding -- not the float evaluation
    {
        const double T[16] = {1.5, 0.25, -0.125, 10000.00043, 0.0, -0.75, 2.0, -12000.0004, 0.3, 0.3, 0.3, 9000.0003, 0.5, -0.5, 7.0, 2.0};
        const float x = 1.2345678f, y = -7.6543210f, z = 3.3333333f;
        float ox, oy, oz;
        mml_world_point(T, x, y, z, ox, oy, oz);
        CHECK(ox == (float)(((T[0] * (double)x + T[1] * (double)y) + T[2] * (double)z) + T[3]));
        CHECK(oy == (float)(((T[4] * (double)x + T[5] * (double)y) + T[6] * (double)z) + T[7]));
        CHECK(oz == (float)(((T[8] * (double)x + T[9] * (double)y) + T[10] * (double)z) + T[11]));
    }
    if (fails) return 1;
    printf("world_map_key_check ok\n");
    return 0;
}
