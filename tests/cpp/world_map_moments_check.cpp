// Stand-alone host program over csrc/world_map_key.h (a surfel map's arithmetic); includes nothing else of the project.
//   world_map_moments_check <input>
// Input, whitespace-separated, every real number in C's hexadecimal notation: leaf, the number of slots; per slot its map, its
// point count, the 16 doubles of its row-major pose and its points x y z intensity (floats, sensor frame).  The points go
// through mml_world_point and mml_wm_classify and, when kept, into their voxel's sums and moments in the order given.
// Output, one line per voxel in ascending key order: key, count, the 12 moments as the 8 hex digits of their bits, the six
// covariance inputs of mml_wm_covariance as hexadecimal doubles.  Returns 1 on a malformed input.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "world_map_key.h"

struct Voxel {
    MmlWmAcc a = {0.f, 0.f, 0.f, 0.f, 0};
    MmlWmMoments m = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
};

static bool next(FILE* f, double& v) {
    char tok[128];
    if (fscanf(f, "%127s", tok) != 1) return false;
    char* end = nullptr;
    v = strtod(tok, &end);
    return end != tok && *end == 0;
}
static unsigned bits(float v) {
    unsigned b;
    memcpy(&b, &v, sizeof(b));
    return b;
}

int main(int argc, char** argv) {
    if (argc != 2) return 1;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 1;
    double v = 0.0, n_slots = 0.0;
    if (!next(f, v) || !next(f, n_slots)) return 1;
    const float leaf = (float)v, inv = mml_wm_inv_leaf(leaf);
    std::map<unsigned long long, Voxel> vox;
    for (int s = 0; s < (int)n_slots; ++s) {
        double map = 0.0, n = 0.0, T[16];
        if (!next(f, map) || !next(f, n)) return 1;
        for (double& t : T)
            if (!next(f, t)) return 1;
        float ox, oy, oz;
        mml_wm_origin(T, ox, oy, oz);
        for (int p = 0; p < (int)n; ++p) {
            double q[4];
            for (double& c : q)
                if (!next(f, c)) return 1;
            float wx, wy, wz;
            mml_world_point(T, (float)q[0], (float)q[1], (float)q[2], wx, wy, wz);
            unsigned long long key = 0;
            if (mml_wm_classify((int)map, wx, wy, wz, (float)q[3], inv, key) != MML_WM_KEPT) continue;
            int m2, i, j, k;
            mml_wm_unkey(key, m2, i, j, k);
            Voxel& x = vox[key];
            mml_wm_add(x.a, wx, wy, wz, (float)q[3]);
            mml_wm_add_moments(x.m, wx, wy, wz, mml_wm_centre(i, leaf), mml_wm_centre(j, leaf), mml_wm_centre(k, leaf), ox, oy, oz);
        }
    }
    fclose(f);
    for (const auto& kv : vox) {
        const MmlWmMoments& m = kv.second.m;
        const float w[12] = {m.sdx, m.sdy, m.sdz, m.vx, m.sxx, m.sxy, m.sxz, m.vy, m.syy, m.syz, m.szz, m.vz};
        printf("%llu %d", kv.first, kv.second.a.n);
        for (float x : w) printf(" %08x", bits(x));
        double c[6];
        mml_wm_covariance(m, kv.second.a.n, c);
        for (double x : c) printf(" %a", x);
        printf("\n");
    }
    return 0;
}
