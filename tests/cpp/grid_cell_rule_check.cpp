// Runs csrc/grid_cell_rule.h, the host's cell-size decisions of a kNN grid build, on cases read from standard input and prints what
// it decided, for tests/test_bank_increment_segmented_host.py to compare with its own restatement.  No HIP, no device.
//   in : per case one line -- the six box floats, the configured cell edge (seven floats as the hex of their bits), max_cells, m,
//        and the occupied-cell counts of five rounds
//   out: per round of the case one line -- round, the cell edge's bits, the three dimensions, ncell, 1 when the next round runs;
//        then "end"
#include <stdio.h>
#include <string.h>

#include "grid_cell_rule.h"

static float from_bits(unsigned u) {
    float f;
    memcpy(&f, &u, sizeof(f));
    return f;
}
static unsigned to_bits(float f) {
    unsigned u;
    memcpy(&u, &f, sizeof(u));
    return u;
}

int main() {
    unsigned b[7];
    long long max_cells;
    int m, occ[5];
    while (scanf("%x %x %x %x %x %x %x %lld %d %d %d %d %d %d", &b[0], &b[1], &b[2], &b[3], &b[4], &b[5], &b[6], &max_cells, &m, &occ[0],
                 &occ[1], &occ[2], &occ[3], &occ[4]) == 14) {
        float bbox[6];
        for (int c = 0; c < 6; ++c) bbox[c] = from_bits(b[c]);
        float cell = from_bits(b[6]);
        for (int round = 0;; ++round) {
            if (round >= 5) return 2;  // (the rule stops after round 4)
            int dim[3];
            mml_grid_fit_cell(bbox, max_cells, cell, dim);
            const int ncell = dim[0] * dim[1] * dim[2];
            const bool again = mml_grid_refine(m, occ[round], round, ncell, max_cells);
            printf("%d %08x %d %d %d %d %d\n", round, to_bits(cell), dim[0], dim[1], dim[2], ncell, again ? 1 : 0);
            if (!again) break;
            cell *= 0.5f;
        }
        printf("end\n");
    }
    return 0;
}
