// csrc/world_map_evict.h on the host, a program of its own: mml_wme_goes and mml_wme_index_box on scripted cases, every case
// printed with its inputs (tests/test_world_map_evict_host.py compares each line with tests/world_map_evict_ref.py).
//   G mode lo0 lo1 lo2 hi0 hi1 hi2 min_count i j k count = goes
//   B leaf lo_xyz[3] hi_xyz[3] (float bits, hex) = rc lo0 lo1 lo2 hi0 hi1 hi2
//   S n_goes_cases n_box_cases
#include <limits>
#include <stdio.h>
#include <string.h>

#include "world_map_evict.h"

static int n_g = 0, n_b = 0;

static mml_wm_evict_rule rule(int mode, int l0, int l1, int l2, int h0, int h1, int h2, int min_count) {
    mml_wm_evict_rule r;
    r.map = 0;
    r.mode = mode;
    r.lo[0] = l0, r.lo[1] = l1, r.lo[2] = l2;
    r.hi[0] = h0, r.hi[1] = h1, r.hi[2] = h2;
    r.min_count = min_count;
    return r;
}
static void g(const mml_wm_evict_rule& r, int i, int j, int k, int count) {
    printf("G %d %d %d %d %d %d %d %d %d %d %d %d = %d\n", r.mode, r.lo[0], r.lo[1], r.lo[2], r.hi[0], r.hi[1], r.hi[2], r.min_count, i, j, k,
           count, (int)mml_wme_goes(r, i, j, k, count));
    ++n_g;
}
static unsigned bits(float v) {
    unsigned b;
    memcpy(&b, &v, sizeof(b));
    return b;
}
static void b(float leaf, float l0, float l1, float l2, float h0, float h1, float h2) {
    const float lo_xyz[3] = {l0, l1, l2}, hi_xyz[3] = {h0, h1, h2};
    int lo[3] = {7, 7, 7}, hi[3] = {7, 7, 7};
    const int rc = mml_wme_index_box(leaf, lo_xyz, hi_xyz, lo, hi);
    printf("B %08x %08x %08x %08x %08x %08x %08x = %d %d %d %d %d %d %d\n", bits(leaf), bits(l0), bits(l1), bits(l2), bits(h0), bits(h1), bits(h2), rc,
           lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    ++n_b;
}

int main() {
    const int H = MML_WM_HALF;
    const int modes[3] = {MML_WM_EVICT_OUTSIDE, MML_WM_EVICT_INSIDE, MML_WM_EVICT_NOBOX};
    // every axis at lo, lo - 1, hi - 1, hi, the other two inside; every mode; a count rule that does not fire and one that does
    for (int m = 0; m < 3; ++m)
        for (int mc = 0; mc <= 4; mc += 4) {
            const mml_wm_evict_rule r = rule(modes[m], -3, 2, -40, 5, 4, -38, mc);
            const int in[3] = {0, 3, -39};
            for (int a = 0; a < 3; ++a) {
                const int at[4] = {r.lo[a], r.lo[a] - 1, r.hi[a] - 1, r.hi[a]};
                for (int e = 0; e < 4; ++e) {
                    int v[3] = {in[0], in[1], in[2]};
                    v[a] = at[e];
                    g(r, v[0], v[1], v[2], 3);
                    g(r, v[0], v[1], v[2], 4);
                }
            }
        }
    // boxes touching the ends of the index range
    for (int m = 0; m < 3; ++m) {
        const mml_wm_evict_rule all = rule(modes[m], -H, -H, -H, H, H, H, 0), low = rule(modes[m], -H, -H, -H, -H + 1, -H + 1, -H + 1, 0),
                                high = rule(modes[m], H - 1, H - 1, H - 1, H, H, H, 0);
        const int at[4] = {-H, -H + 1, H - 2, H - 1};
        for (int e = 0; e < 4; ++e) {
            g(all, at[e], at[e], at[e], 1);
            g(low, at[e], at[e], at[e], 1);
            g(high, at[e], at[e], at[e], 1);
            g(low, at[e], -H, -H, 1);
            g(high, H - 1, H - 1, at[e], 1);
        }
    }
    // empty boxes under both modes (and NOBOX): lo == hi, lo > hi, on one axis and on all
    for (int m = 0; m < 3; ++m) {
        const mml_wm_evict_rule e0 = rule(modes[m], 2, -5, -5, 2, 5, 5, 0), e1 = rule(modes[m], -5, 3, -5, 5, 1, 5, 0),
                                e2 = rule(modes[m], 0, 0, 0, 0, 0, 0, 0), e3 = rule(modes[m], H, H, H, -H, -H, -H, 1);
        const int at[3] = {-1, 0, 2};
        for (int e = 0; e < 3; ++e) {
            g(e0, at[e], 0, 0, 1);
            g(e1, 0, at[e], 0, 1);
            g(e2, at[e], at[e], at[e], 1);
            g(e3, at[e], 0, at[e], 1);
        }
    }
    // NOBOX does not read the box
    g(rule(MML_WM_EVICT_NOBOX, 0, 0, 0, 10, 10, 10, 0), 5, 5, 5, 1);
    g(rule(MML_WM_EVICT_NOBOX, 0, 0, 0, 10, 10, 10, 3), 5, 5, 5, 2);
    g(rule(MML_WM_EVICT_NOBOX, 0, 0, 0, 10, 10, 10, 3), 50, 5, 5, 3);
    // min_count 0, 1, 2 with the count equal to it and one below, a voxel that the box keeps, every mode
    for (int m = 0; m < 3; ++m)
        for (int mc = 0; mc <= 2; ++mc) {
            const bool out = modes[m] == MML_WM_EVICT_INSIDE;
            const mml_wm_evict_rule r = rule(modes[m], -2, -2, -2, 2, 2, 2, mc);
            g(r, out ? 9 : 0, 0, 0, mc);
            g(r, out ? 9 : 0, 0, 0, mc - 1);
            g(r, out ? 0 : 9, 0, 0, mc);      // (... and one that the box evicts whatever the count)
        }
    g(rule(MML_WM_EVICT_OUTSIDE, -2, -2, -2, 2, 2, 2, 3), 0, 0, 0, std::numeric_limits<int>::max());

    // metric boxes: corners on voxel faces, negative coordinates, inside a voxel
    const float leaves[4] = {0.5f, 0.1f, 0.3f, 2.0f};
    for (int l = 0; l < 4; ++l) {
        const float f = leaves[l];
        b(f, 0.f, 0.f, 0.f, f, 2.f * f, 3.f * f);
        b(f, -f, -2.f * f, -3.f * f, 0.f, 0.f, 0.f);
        b(f, -0.f, 0.f, -0.f, -0.f, 0.f, -0.f);
        b(f, -1.25f, -7.3f, -0.01f, 1.25f, 7.3f, 0.01f);
        b(f, 10.f * f, -10.f * f, 7.f * f, 11.f * f, -9.f * f, 7.f * f);
        b(f, 3.f, 3.f, 3.f, -3.f, -3.f, -3.f);          // (hi below lo: an empty index box)
        b(f, -1e-30f, 1e-30f, -1e-45f, 1e-30f, -1e-30f, 1e-45f);
        // the ends of the index range, and past them: clamped
        b(f, -(float)MML_WM_HALF * f, (float)(MML_WM_HALF - 1) * f, (float)MML_WM_HALF * f, (float)(MML_WM_HALF - 1) * f, (float)MML_WM_HALF * f, 0.f);
        b(f, -1e9f, -1e30f, -3.4e38f, 1e9f, 1e30f, 3.4e38f);
        b(f, 1e30f, 1e30f, 1e30f, -1e30f, -1e30f, -1e30f);
    }
    b(1e-30f, -1.f, 0.f, 1.f, -1.f, 0.f, 1.f);          // (products overflow to infinity: clamped)
    b(1e-45f, -1.f, 0.f, 1.f, -1.f, 0.f, 1.f);          // (the inverse leaf is infinite; 0 x inf is no number: the low end)
    // refused: a coordinate or the leaf not finite, the leaf not positive -- nothing is written
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    b(0.5f, nan, 0.f, 0.f, 1.f, 1.f, 1.f);
    b(0.5f, 0.f, 0.f, 0.f, 1.f, inf, 1.f);
    b(0.5f, 0.f, 0.f, -inf, 1.f, 1.f, 1.f);
    b(0.f, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
    b(-0.5f, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
    b(nan, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
    b(inf, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
    printf("S %d %d\n", n_g, n_b);
    return 0;
}
