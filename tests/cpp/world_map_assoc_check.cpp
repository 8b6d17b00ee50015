// world_map_assoc_check.cpp -- csrc/world_map_assoc.h on the host, a program of its own (built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_world_map_assoc_host.py): scripted and generated cases through the header's voxel,
// candidate, choice and factor functions, every case printed with its inputs and its result as bit patterns, so that the test can
// run the same inputs through the numpy restatement (tests/world_map_assoc_ref.py) and compare bit for bit.
//   C map neighbourhood min_points min_planarity max_plane_dist inv | 12 doubles of T | 3 floats of f | candidates
//   V i j k count | sum x y z | surfel nx ny nz planarity           (one line per voxel the map holds)
//   R status | ori 3, proj 3, omega 3, error (doubles)              status: 0 skipped, 1 no candidate, 2 planarity, 3 distance, 4 factor
//   S the five status counts                                        (the last line)
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <vector>

#include "world_map_assoc.h"

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
    double T[12];
    float f[3];
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
// a small generator of its own (the test reads the printed inputs, not this sequence)
unsigned long long g_state = 0x9E3779B97F4A7C15ull;
double rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}
int rndi(int n) { return (int)(rnd() * n) % n; }

int g_status[5];

void run(const Case& c) {
    printf("C %d %d %d %08x %016llx %08x |", c.map, c.nb, c.min_points, fb(c.min_planarity), db(c.max_dist), fb(c.inv));
    for (int a = 0; a < 12; ++a) printf(" %016llx", db(c.T[a]));
    printf(" | %08x %08x %08x | %zu\n", fb(c.f[0]), fb(c.f[1]), fb(c.f[2]), c.vox.size());
    std::map<unsigned long long, long long> table;  // key -> index in c.vox
    for (size_t r = 0; r < c.vox.size(); ++r) {
        const Voxel& v = c.vox[r];
        printf("V %d %d %d %d | %08x %08x %08x | %08x %08x %08x %08x\n", v.i, v.j, v.k, v.count, fb(v.sx), fb(v.sy), fb(v.sz), fb(v.nx), fb(v.ny), fb(v.nz),
               fb(v.planarity));
        table[mml_wm_key(c.map, v.i, v.j, v.k)] = (long long)r;
    }
    float wx, wy, wz;
    mml_world_point(c.T, c.f[0], c.f[1], c.f[2], wx, wy, wz);
    int vi = 0, vj = 0, vk = 0, status = 0;
    MmlWmaFactor F;
    memset(&F, 0, sizeof(F));
    if (mml_wma_voxel(wx, wy, wz, c.inv, vi, vj, vk)) {
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
        status = 1;
        if (best.at >= 0) {
            const Voxel* win = &c.vox[(size_t)best.at];
            status = 2;
            if (!(win->planarity < c.min_planarity)) {
                status = 3;
                if (mml_wma_factor(c.T, c.f[0], c.f[1], c.f[2], wx, wy, wz, best.cx, best.cy, best.cz, win->nx, win->ny, win->nz, win->planarity,
                                   c.min_planarity, c.max_dist, F))
                    status = 4;
            }
        }
    }
    g_status[status]++;
    printf("R %d |", status);
    if (status == 4) {
        for (int a = 0; a < 3; ++a) printf(" %016llx", db((double)F.ori[a]));
        for (int a = 0; a < 3; ++a) printf(" %016llx", db(F.proj[a]));
        for (int a = 0; a < 3; ++a) printf(" %016llx", db((double)F.omega[a]));
        printf(" %016llx", db(F.error));
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
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    memcpy(c.T, I, sizeof(I));
    c.f[0] = c.f[1] = c.f[2] = 0.f;
    return c;
}
// a voxel whose centroid is (cx, cy, cz) exactly when the values and the count allow it
Voxel voxel(int i, int j, int k, int count, float cx, float cy, float cz, float nx, float ny, float nz, float planarity) {
    return Voxel{i, j, k, count, cx * (float)count, cy * (float)count, cz * (float)count, nx, ny, nz, planarity};
}
}  // namespace

int main() {
    const float leaf = 0.5f;
    // ---- scripted ----
    {  // a tie in r2 between two voxels, broken by the key; with neighbourhood 0 the point's own voxel alone
        Case c = base(leaf);
        c.f[0] = 0.5f;  // on the face x = 0.5: its voxel is (1, 0, 0)
        c.f[1] = c.f[2] = 0.25f;
        c.vox.push_back(voxel(1, 0, 0, 8, 0.75f, 0.25f, 0.25f, 0.f, 0.f, 1.f, 0.9f));
        c.vox.push_back(voxel(0, 0, 0, 8, 0.25f, 0.25f, 0.25f, 0.f, 1.f, 0.f, 0.9f));
        run(c);
        c.nb = 0;
        run(c);
        c.nb = 1;
        c.vox.push_back(voxel(1, 0, -1, 8, 0.75f, 0.25f, 0.25f, 1.f, 0.f, 0.f, 0.9f));  // a third at the same distance, in another k layer
        c.vox.push_back(voxel(0, -1, 0, 8, 0.25f, 0.25f, 0.25f, 1.f, 0.f, 0.f, 0.9f));
        run(c);
    }
    for (int axis = 0; axis < 3; ++axis)  // a point exactly on a voxel face of every axis, the nearer centroid in the neighbour
        for (int side = 0; side < 2; ++side) {
            Case c = base(leaf);
            c.f[0] = c.f[1] = c.f[2] = 0.3f;
            c.f[axis] = side ? 0.5f : 0.0f;
            int a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
            a[axis] = side ? 1 : 0;
            b[axis] = a[axis] - 1;
            float ca[3] = {0.3f, 0.3f, 0.3f}, cb[3] = {0.3f, 0.3f, 0.3f};
            ca[axis] = c.f[axis] + 0.2f;
            cb[axis] = c.f[axis] - 0.1f;
            c.vox.push_back(voxel(a[0], a[1], a[2], 6, ca[0], ca[1], ca[2], axis == 0, axis == 1, axis == 2, 0.8f));
            c.vox.push_back(voxel(b[0], b[1], b[2], 6, cb[0], cb[1], cb[2], axis == 0, axis == 1, axis == 2, 0.8f));
            run(c);
        }
    for (int e = 0; e < 2; ++e)  // the index-range edges: the neighbours beyond them are not candidates
        for (int axis = 0; axis < 3; ++axis) {
            Case c = base(leaf);
            const int idx = e ? MML_WM_HALF - 1 : -MML_WM_HALF;
            c.f[0] = c.f[1] = c.f[2] = 0.2f;
            c.f[axis] = ((float)idx + 0.5f) * leaf;
            int a[3] = {0, 0, 0};
            a[axis] = idx;
            float cen[3] = {0.2f, 0.2f, 0.2f};
            cen[axis] = c.f[axis];
            c.vox.push_back(voxel(a[0], a[1], a[2], 7, cen[0], cen[1], cen[2], axis == 0, axis == 1, axis == 2, 1.0f));
            run(c);
            c.f[axis] = ((float)(e ? MML_WM_HALF : -MML_WM_HALF - 1) + 0.5f) * leaf;  // the feature itself beyond the range: skipped
            run(c);
        }
    {  // map 1023: the voxel whose key is the free marker is no candidate, its neighbour is
        Case c = base(leaf);
        c.map = 1023;
        const int m = MML_WM_HALF - 1;
        c.f[0] = c.f[1] = c.f[2] = ((float)m + 0.5f) * leaf;
        c.vox.push_back(voxel(m, m, m, 9, c.f[0], c.f[1], c.f[2], 0.f, 0.f, 1.f, 1.0f));
        run(c);
        c.vox.push_back(voxel(m - 1, m, m, 9, c.f[0] - 0.5f, c.f[1], c.f[2], 0.f, 0.f, 1.f, 1.0f));
        run(c);
    }
    {  // not finite
        Case c = base(leaf);
        c.vox.push_back(voxel(0, 0, 0, 9, 0.2f, 0.2f, 0.2f, 0.f, 0.f, 1.f, 1.0f));
        const float zero = 0.f;
        c.f[1] = zero / zero;
        run(c);
        c.f[1] = 1.0f / zero;
        run(c);
        c.f[1] = 0.f;
        c.T[3] = 1e300;  // the world point overflows to infinity
        run(c);
    }
    {  // a winner that fails each gate -- and no second choice although another voxel would pass
        Case c = base(leaf);
        c.f[0] = c.f[1] = 0.2f;
        c.f[2] = 0.3f;
        c.vox.push_back(voxel(0, 0, 0, 9, 0.2f, 0.2f, 0.2f, 0.f, 0.f, 1.f, 0.49f));   // planarity just below
        c.vox.push_back(voxel(1, 0, 0, 9, 0.7f, 0.2f, 0.3f, 0.f, 0.f, 1.f, 0.9f));
        run(c);
        c.vox[0].planarity = 0.5f;  // exactly at the gate: passes
        run(c);
        c.max_dist = 0.05;          // |d| = 0.1 (as floats) above the gate
        run(c);
        c.max_dist = (double)(0.3f) - (double)(0.2f);  // |d| exactly at the gate: passes
        run(c);
        c.min_points = 10;          // nobody takes part
        run(c);
        c.min_points = 9;
        c.vox[0].count = 8;         // the nearer voxel has min_points - 1 points: the other one wins
        run(c);
    }
    // ---- generated: coordinates on a grid of 1/16 m so that ties and points on faces occur, poses near the identity ----
    for (int n = 0; n < 400; ++n) {
        Case c = base(leaf);
        c.map = rndi(3);
        c.nb = n % 5 != 0;
        c.min_points = 3 + rndi(4);
        c.min_planarity = (float)(0.25 * rndi(4));
        c.max_dist = 0.0625 * (1 + rndi(8));
        const bool grid = n % 2 == 0;
        if (!grid)
            for (int a = 0; a < 12; ++a) c.T[a] += (rnd() - 0.5) * 0.1;
        for (int a = 0; a < 3; ++a) {
            c.T[4 * a + 3] = grid ? 0.0625 * (rndi(64) - 32) : (rnd() - 0.5) * 4.0;
            c.f[a] = grid ? 0.0625f * (float)(rndi(64) - 32) : (float)((rnd() - 0.5) * 4.0);
        }
        float wx, wy, wz;
        mml_world_point(c.T, c.f[0], c.f[1], c.f[2], wx, wy, wz);
        int vi, vj, vk;
        if (mml_wma_voxel(wx, wy, wz, c.inv, vi, vj, vk))
            for (int dk = -1; dk <= 1; ++dk)
                for (int dj = -1; dj <= 1; ++dj)
                    for (int di = -1; di <= 1; ++di) {
                        if (rndi(3) == 0) continue;
                        const int count = 1 + rndi(8);
                        float cen[3];
                        const int ijk[3] = {vi + di, vj + dj, vk + dk};
                        for (int a = 0; a < 3; ++a)
                            cen[a] = grid ? ((float)ijk[a] + 0.25f * (float)(1 + rndi(3))) * leaf : ((float)ijk[a] + (float)rnd()) * leaf;
                        float nrm[3] = {(float)(rnd() - 0.5), (float)(rnd() - 0.5), (float)(rnd() - 0.5)};
                        if (grid) {
                            nrm[0] = nrm[1] = nrm[2] = 0.f;
                            nrm[rndi(3)] = rndi(2) ? 1.f : -1.f;
                        }
                        Voxel v = voxel(ijk[0], ijk[1], ijk[2], grid ? 8 >> rndi(3) : count, cen[0], cen[1], cen[2], nrm[0], nrm[1], nrm[2], (float)(0.125 * rndi(9)));
                        if (grid && v.count < c.min_points) v.count = 8;
                        if (grid) {
                            v.sx = cen[0] * (float)v.count;
                            v.sy = cen[1] * (float)v.count;
                            v.sz = cen[2] * (float)v.count;
                        }
                        c.vox.push_back(v);
                    }
        run(c);
    }
    printf("S %d %d %d %d %d\n", g_status[0], g_status[1], g_status[2], g_status[3], g_status[4]);
    return 0;
}
