// grid_cell_rule.h -- the host's cell-size decisions of a kNN grid build, the one definition behind the one grid builder
// (map_assoc.hip mml_build_grids: a set map's one cloud, an increment's 2 n).  Plain C++ without HIP: a host program can include this file alone and check
// the rule on its own (tests/test_bank_increment_segmented_host.py).
//   The configured cell edge suits a voxel-filtered map (<= 1 point per leaf).  A round of a build fits the cell to the cloud's
//   bounding box and the cell budget (mml_grid_fit_cell), sorts the points by cell and counts the occupied cells; if the cloud is
//   denser than 12 points per occupied cell on average, the cell is halved and the round repeated (mml_grid_refine), five rounds
//   at the most and never past the budget.
#ifndef MML_GRID_CELL_RULE_H
#define MML_GRID_CELL_RULE_H

#include <math.h>

// cells a grid over a map of at most max_map_points points may have (its cell_start array holds two more ints)
inline long long mml_grid_max_cells(int max_map_points) { return (long long)4 * max_map_points + 4096; }

// The cells per axis of the box bbox (min x, y, z, max x, y, z) at edge `cell`; while they exceed max_cells the edge grows by 1.26
// (a factor of two in volume).  `cell` holds the edge that fits on return.
inline void mml_grid_fit_cell(const float bbox[6], long long max_cells, float& cell, int dim[3]) {
    for (;;) {
        long long total = 1;
        for (int c = 0; c < 3; ++c) {
            dim[c] = (int)floorf((bbox[3 + c] - bbox[c]) / cell) + 1;
            if (dim[c] < 1) dim[c] = 1;
            total *= dim[c];
        }
        if (total <= max_cells) break;
        cell *= 1.26f;
    }
}

// After round `round` (0-based) of a build over m points that found `occ` occupied cells among ncell: true when the next round
// runs, at `cell * 0.5f`.
inline bool mml_grid_refine(int m, int occ, int round, int ncell, long long max_cells) {
    const double per_cell = (double)m / (occ > 0 ? occ : 1);
    const long long next_total = (long long)ncell * 8;
    return !(per_cell <= 12.0 || round >= 4 || next_total > max_cells);
}

#endif
