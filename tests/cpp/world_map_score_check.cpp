// world_map_score_check.cpp -- csrc/world_map_score.h on the host, a program of its own (built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_world_map_score_host.py): scripted and generated cases -- a small stack of features, a
// pose, the voxels a map holds -- through the header's functions exactly as k_wm_score calls them, every case printed with its
// inputs and its result as bit patterns, so that the test can run the same inputs through the numpy restatement
// (tests/world_map_score_ref.py) and compare bit for bit.
//   C map neighbourhood min_points min_planarity max_plane_dist inv stride | 12 doubles of T | features voxels
//   F x y z                                                          (one line per feature of the stack)
//   V i j k count | sum x y z | surfel nx ny nz planarity            (one line per voxel the map holds)
//   R score_q n_match n_scored | status q ...                        (per feature looked at: 0 skipped, 1 none, 2 planarity, 3 distance, 4 match)
//   S the five status counts                                         (the last line)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <vector>

#include "world_map_score.h"

namespace {
struct Voxel {
    int i, j, k, count;
    float sx, sy, sz, nx, ny, nz, planarity;
};
struct Case {
    int map, nb, min_points;
    float min_planarity;
    double max_dist;
    float inv;
    int stride;
    double T[12];
    std::vector<float> f;  // 3 per feature
    std::vector<Voxel> vox;
};
uint32_t fb(float v) {
    uint32_t b;
    memcpy(&b, &v, sizeof(b));
    return b;
}
unsigned long long db(double v) {
    unsigned long long b;
    memcpy(&b, &v, sizeof(b));
    return b;
}
unsigned long long g_state = 0x2545F4914F6CDD1Dull;
double rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
int rndi(int n) { return (int)(rnd() * n) % n; }

int g_status[5];

void run(const Case& c) {
    const int nf = (int)c.f.size() / 3;
    printf("C %d %d %d %08x %016llx %08x %d |", c.map, c.nb, c.min_points, fb(c.min_planarity), db(c.max_dist), fb(c.inv), c.stride);
    for (int a = 0; a < 12; ++a) printf(" %016llx", db(c.T[a]));
    printf(" | %d %zu\n", nf, c.vox.size());
    for (int s = 0; s < nf; ++s) printf("F %08x %08x %08x\n", fb(c.f[3 * s]), fb(c.f[3 * s + 1]), fb(c.f[3 * s + 2]));
    std::map<unsigned long long, long long> table;  // key -> index in c.vox
    for (size_t r = 0; r < c.vox.size(); ++r) {
        const Voxel& v = c.vox[r];
        printf("V %d %d %d %d | %08x %08x %08x | %08x %08x %08x %08x\n", v.i, v.j, v.k, v.count, fb(v.sx), fb(v.sy), fb(v.sz), fb(v.nx), fb(v.ny), fb(v.nz),
               fb(v.planarity));
        table[mml_wm_key(c.map, v.i, v.j, v.k)] = (long long)r;
    }
    MmlWmsAcc acc;
    mml_wms_init(acc);
    std::vector<int> status;
    std::vector<unsigned long long> q;
    const int n = mml_wms_count(nf, c.stride);
    for (int t = 0; t < n; ++t) {
        const float* f = &c.f[3 * (size_t)mml_wms_feature(t, c.stride)];
        float wx, wy, wz;
        mml_world_point(c.T, f[0], f[1], f[2], wx, wy, wz);
        int vi = 0, vj = 0, vk = 0;
        if (!mml_wma_voxel(wx, wy, wz, c.inv, vi, vj, vk)) {
            status.push_back(MML_WMS_SKIPPED);
            q.push_back(0);
            continue;
        }
        MmlWmaBest best;
        mml_wma_best_init(best);
        for (int dk = -1; dk <= 1; ++dk)
            for (int dj = -1; dj <= 1; ++dj)
                for (int di = -1; di <= 1; ++di) {
                    if (!c.nb && (di || dj || dk)) continue;
                    unsigned long long key;
                    if (!mml_wma_candidate(c.map, vi + di, vj + dj, vk + dk, key)) continue;
                    const auto it = table.find(key);
                    if (it == table.end() || c.vox[(size_t)it->second].count < c.min_points) continue;
                    const Voxel& v = c.vox[(size_t)it->second];
                    const MmlWmAcc a = {v.sx, v.sy, v.sz, 0.f, v.count};
                    float cen[4];
                    mml_wm_centroid(a, cen);
                    mml_wma_offer(best, mml_wma_r2(wx, wy, wz, cen[0], cen[1], cen[2]), key, it->second, v.count, cen[0], cen[1], cen[2]);
                }
        float nx = 0.f, ny = 0.f, nz = 0.f, pl = 0.f;
        if (best.at >= 0) {
            const Voxel& w = c.vox[(size_t)best.at];
            nx = w.nx, ny = w.ny, nz = w.nz, pl = w.planarity;
        }
        const unsigned long long before = acc.score_q;
        status.push_back(mml_wms_add(acc, wx, wy, wz, best, nx, ny, nz, pl, c.min_planarity, c.max_dist));
        q.push_back(acc.score_q - before);
    }
    printf("R %llu %d %d |", acc.score_q, acc.n_match, acc.n_scored);
    for (size_t t = 0; t < status.size(); ++t) {
        printf(" %d %llu", status[t], q[t]);
        g_status[status[t]]++;
    }
    printf("\n");
}

Case base(float leaf) {
    Case c;
    c.map = 0;
    c.nb = 1;
    c.min_points = 5;
    c.min_planarity = 0.5f;
    c.max_dist = (double)leaf;
    c.inv = mml_wm_inv_leaf(leaf);
    c.stride = 1;
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    memcpy(c.T, I, sizeof(I));
    return c;
}
void feature(Case& c, float x, float y, float z) {
    c.f.push_back(x);
    c.f.push_back(y);
    c.f.push_back(z);
}
Voxel voxel(int i, int j, int k, int count, float cx, float cy, float cz, float nx, float ny, float nz, float planarity) {
    return Voxel{i, j, k, count, cx * (float)count, cy * (float)count, cz * (float)count, nx, ny, nz, planarity};
}
}  // namespace

int main() {
    const float leaf = 0.5f;
    // ---- scripted: one horizontal patch at z = 0.25 in voxel (0, 0, 0), the gate at 0.125 ----
    {
        Case c = base(leaf);
        c.max_dist = 0.125;
        c.vox.push_back(voxel(0, 0, 0, 8, 0.25f, 0.25f, 0.25f, 0.f, 0.f, 1.f, 0.9f));
        feature(c, 0.25f, 0.25f, 0.25f);                 // |d| = 0: q = 65536
        feature(c, 0.25f, 0.25f, 0.25f + 0.1249f);       // just inside the gate
        feature(c, 0.25f, 0.25f, 0.25f + 0.1251f);       // just outside it
        feature(c, 0.25f, 0.25f, 0.375f);                // |d| exactly max_plane_dist: q = 0, still a match
        feature(c, 0.25f, 0.25f, 0.125f);                // the same below the plane
        run(c);
        c.vox[0].planarity = 0.49f;                      // the planarity gate fails for all of them
        run(c);
        c.vox[0].planarity = 0.9f;
        const float zero = 0.f;
        feature(c, zero / zero, 0.f, 0.f);               // skipped: not finite
        feature(c, ((float)MML_WM_HALF + 0.5f) * leaf, 0.f, 0.f);  // skipped: beyond the index range
        feature(c, 3.25f, 0.25f, 0.25f);                 // looked at, no candidate
        run(c);
        for (int stride = 1; stride <= 9; ++stride) {    // 8 features: strides that leave 8, 4, 3, 2, 2, 2, 2, 1, 1
            c.stride = stride;
            run(c);
        }
        c.f.resize(3);                                   // one feature: every stride leaves it
        c.stride = 1;
        run(c);
        c.stride = 4;
        run(c);
        c.f.clear();                                     // none: a stride leaves zero
        c.stride = 1;
        run(c);
        c.stride = 3;
        run(c);
    }
    {  // a pose with an entry that is not a number: every feature is skipped
        Case c = base(leaf);
        c.vox.push_back(voxel(0, 0, 0, 8, 0.25f, 0.25f, 0.25f, 0.f, 0.f, 1.f, 0.9f));
        feature(c, 0.25f, 0.25f, 0.25f);
        feature(c, 0.2f, 0.3f, 0.2f);
        const double zero = 0.0;
        c.T[5] = zero / zero;
        run(c);
        c.T[5] = 1.0;
        c.T[11] = 1e300;
        run(c);
    }
    {  // a surfel whose normal is not a number passes the comparison of the gate (as in mml_wma_factor): a match of q = 0
        Case c = base(leaf);
        const float zero = 0.f;
        c.vox.push_back(voxel(0, 0, 0, 8, 0.25f, 0.25f, 0.25f, zero / zero, 0.f, 1.f, 0.9f));
        feature(c, 0.25f, 0.25f, 0.3f);
        run(c);
    }
    // ---- generated: stacks of up to 12 features on a grid of 1/16 m or free, poses near the identity, the voxels around them ----
    for (int n = 0; n < 300; ++n) {
        Case c = base(leaf);
        c.map = rndi(3);
        c.nb = n % 5 != 0;
        c.min_points = 3 + rndi(4);
        c.min_planarity = (float)(0.25 * rndi(4));
        c.max_dist = 0.0625 * (1 + rndi(8));
        c.stride = 1 + rndi(3);
        const bool grid = n % 2 == 0;
        if (!grid)
            for (int a = 0; a < 12; ++a) c.T[a] += (rnd() - 0.5) * 0.1;
        for (int a = 0; a < 3; ++a) c.T[4 * a + 3] = grid ? 0.0625 * (rndi(64) - 32) : (rnd() - 0.5) * 4.0;
        const int nf = rndi(13);
        for (int s = 0; s < nf; ++s)
            feature(c, grid ? 0.0625f * (float)(rndi(32) - 16) : (float)(rnd() - 0.5) * 2.0f, grid ? 0.0625f * (float)(rndi(32) - 16) : (float)(rnd() - 0.5) * 2.0f,
                    grid ? 0.0625f * (float)(rndi(32) - 16) : (float)(rnd() - 0.5) * 2.0f);
        std::map<unsigned long long, int> seen;
        for (int s = 0; s < nf; ++s) {
            float wx, wy, wz;
            mml_world_point(c.T, c.f[3 * s], c.f[3 * s + 1], c.f[3 * s + 2], wx, wy, wz);
            int vi, vj, vk;
            if (!mml_wma_voxel(wx, wy, wz, c.inv, vi, vj, vk)) continue;
            for (int dk = -1; dk <= 1; ++dk)
                for (int dj = -1; dj <= 1; ++dj)
                    for (int di = -1; di <= 1; ++di) {
                        const int ijk[3] = {vi + di, vj + dj, vk + dk};
                        if (rndi(3) == 0 || seen.count(mml_wm_key(c.map, ijk[0], ijk[1], ijk[2]))) continue;
                        seen[mml_wm_key(c.map, ijk[0], ijk[1], ijk[2])] = 1;
                        float cen[3];
                        for (int a = 0; a < 3; ++a) cen[a] = grid ? ((float)ijk[a] + 0.25f * (float)(1 + rndi(3))) * leaf : ((float)ijk[a] + (float)rnd()) * leaf;
                        float nrm[3] = {(float)(rnd() - 0.5), (float)(rnd() - 0.5), (float)(rnd() - 0.5)};
                        if (grid) {
                            nrm[0] = nrm[1] = nrm[2] = 0.f;
                            nrm[rndi(3)] = rndi(2) ? 1.f : -1.f;
                        }
                        const int count = grid ? 8 >> rndi(2) : 1 + rndi(8);
                        c.vox.push_back(voxel(ijk[0], ijk[1], ijk[2], count, cen[0], cen[1], cen[2], nrm[0], nrm[1], nrm[2], (float)(0.125 * rndi(9))));
                    }
        }
        run(c);
    }
    printf("S %d %d %d %d %d\n", g_status[0], g_status[1], g_status[2], g_status[3], g_status[4]);
    return 0;
}
