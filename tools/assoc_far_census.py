"""Census of the association's far queries (numpy; no device needed with --cpu-extractor): which share of the 5-NN queries goes
beyond ring 1, at which shell they finish, how many end without a factor, and how many (y, z) rows of the shells >= 2 a query
visits -- as the search stood (bound = the fifth distance so far, unbounded while fewer than five candidates are known) and with
the bound clipped by the gate (min(bound, thres_dist): the sphere clip of k_associate_hard).

    python tools/assoc_far_census.py --cpu-extractor DIR:MODULE [--scans 8] [--tiles 9] > profiles/assoc_far_census.txt

The feature stacks come from the product's own extraction (a Context on device 0) or, with --cpu-extractor, from a CPU
restatement of it: a module MODULE in DIR with extract_velo, extract_livox, undistort and voxel_downsample, such as the one
the test suite checks the product against (profiles/assoc_far_census.txt was made that way).

Input: config 1 of bench.py -- a few of its scans from `synth`, a map built as bench.py::build_maps builds it (features of
the 8 preceding scans in the world frame, voxel-filtered, grown by tiled replication) at reduced tiling, the bench's perturbed
start poses.  The grid mapping, the stop rule (knn_done) and the row rule (scan_shell_row) of csrc/knn5_dev.h are restated
here.  Rows are counted with the bound a query has at the START of each shell, so the counts are upper bounds of what the
kernel visits (its bound tightens inside a shell as well); the same holds for both variants."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = np.float32
INF = float("inf")


# ---- the grid mapping and the rules of csrc/knn5_dev.h, restated -------------------------------------------------------
def grid_of(points, cell):
    """origin (bounding-box minimum), cell edge, cells per axis: build_grid_into without its density / budget adjustments."""
    lo, hi = points.min(0).astype(F), points.max(0).astype(F)
    dims = np.maximum(np.floor((hi - lo) / F(cell)).astype(int) + 1, 1)
    return dict(origin=lo, cell=float(F(cell)), dims=dims)


def cell_coords(g, p):
    """Clamped cell of every point (cell_coord)."""
    c = np.floor((np.asarray(p, F) - g["origin"]) * F(1.0 / g["cell"])).astype(int)
    return np.clip(c, 0, g["dims"] - 1)


def query_cell(g, q):
    """Home cell (unclamped), position in cell units, inset (distance to the nearest face of the home cell)."""
    f = (np.asarray(q, np.float64) - g["origin"]) / g["cell"]
    h = np.floor(f).astype(int)
    inset = max(0.0, float(np.min(np.minimum(f - h, h + 1 - f))))
    return h, f, inset


def rmax_of(g, thres):
    return int(np.ceil(np.sqrt(thres) / g["cell"])) + 1


def knn_done(g, inset, r, d5, thres):
    """True when the search may stop after shell r: the fifth distance lies inside the visited radius, or that radius has
    reached the gate."""
    rho = (r + inset) * g["cell"] - 1e-3 * g["cell"]
    if not rho > 0:
        return False
    return d5 < rho * rho or rho * rho >= thres


def shell_rows(dims, h, r):
    """The in-grid (y, z) rows of shell r around home cell h."""
    ylo, yhi = max(h[1] - r, 0), min(h[1] + r, dims[1] - 1)
    zlo, zhi = max(h[2] - r, 0), min(h[2] + r, dims[2] - 1)
    return [(y, z) for z in range(zlo, zhi + 1) for y in range(ylo, yhi + 1)]


def row_cells(dims, h, f, r, y, z, bound_cells):
    """The x cells of row (y, z) of shell r that a search with the bound `bound_cells` (a distance in cell units, inf: none)
    reads: the span on a face row, the two end cells otherwise; None when the whole row lies beyond the bound."""
    xlo, xhi = -1, dims[0]
    if bound_cells < INF:
        gy = y - f[1] if y > h[1] else (f[1] - (y + 1) if y < h[1] else 0.0)
        gz = z - f[2] if z > h[2] else (f[2] - (z + 1) if z < h[2] else 0.0)
        reach = bound_cells * np.sqrt(1.00001) + 4e-3
        w2 = reach * reach - (gy * gy + gz * gz)
        if w2 < 0:
            return None
        w = np.sqrt(w2)
        xlo, xhi = int(np.floor(max(f[0] - w, -1.0))), int(np.floor(min(f[0] + w, float(dims[0]))))
    x0, x1 = h[0] - r, h[0] + r
    if z in (h[2] - r, h[2] + r) or y in (h[1] - r, h[1] + r):
        return list(range(max(x0, 0, xlo), min(x1, dims[0] - 1, xhi) + 1))
    out = []
    if 0 <= x0 < dims[0] and x0 >= xlo:
        out.append(x0)
    if 0 <= x1 < dims[0] and x1 != x0 and x1 <= xhi:
        out.append(x1)
    return out


def count_rows(occ, h, f, r, bound_cells):
    """(rows visited, of them without a point in the cells read) of shell r; occ: points per cell, indexed [x, y, z]."""
    dims = occ.shape
    visited = empty = 0
    for y, z in shell_rows(dims, h, r):
        cells = row_cells(dims, h, f, r, y, z, bound_cells)
        if cells is None:
            continue
        visited += 1
        if not any(occ[x, y, z] for x in cells):
            empty += 1
    return visited, empty


# ---- the census ----------------------------------------------------------------------------------------------------
def census_kind(name, feats_world, map_pts, cell, thres, out):
    g = grid_of(map_pts, cell)
    mc = cell_coords(g, map_pts)
    occ = np.zeros(tuple(g["dims"]), np.int32)
    np.add.at(occ, (mc[:, 0], mc[:, 1], mc[:, 2]), 1)
    rmax = rmax_of(g, thres)
    n = far = nofac = 0
    finish = {}
    rows_now = rows_clip = empty_now = empty_clip = rows_all = 0
    for q in feats_world:
        n += 1
        h, f, inset = query_cell(g, q)
        cheb = np.abs(mc - h).max(1)
        d2 = ((map_pts - q.astype(F)) ** 2).sum(1, dtype=F)

        def d5_within(r):
            d = d2[cheb <= r]
            return float(np.partition(d, 4)[4]) if len(d) >= 5 else INF
        if knn_done(g, inset, 0, d5_within(0), thres) or knn_done(g, inset, 1, d5_within(1), thres) or rmax < 2:
            continue
        far += 1
        d5 = d5_within(1)
        r_end = rmax
        for r in range(2, rmax + 1):
            b_now = np.sqrt(d5) / g["cell"] if d5 < INF else INF
            b_clip = np.sqrt(min(d5, thres)) / g["cell"]
            v, e = count_rows(occ, h, f, r, b_now)
            vc, ec = count_rows(occ, h, f, r, b_clip)
            rows_all += len(shell_rows(occ.shape, h, r))
            rows_now, empty_now, rows_clip, empty_clip = rows_now + v, empty_now + e, rows_clip + vc, empty_clip + ec
            d5 = d5_within(r)
            if knn_done(g, inset, r, d5, thres):
                r_end = r
                break
        finish[r_end] = finish.get(r_end, 0) + 1
        if not d5 < thres:
            nofac += 1
    p = lambda *a: print(*a, file=out)
    p("%s: map %d points, cell %.2f m, grid %s, last shell %d" % (name, len(map_pts), g["cell"], "x".join(map(str, g["dims"])), rmax))
    p("  queries %d, far (beyond ring 1) %d = %.2f %%" % (n, far, 100.0 * far / max(n, 1)))
    if far:
        p("  finishing shell: " + ", ".join("%d: %d (%.1f %%)" % (r, c, 100.0 * c / far) for r, c in sorted(finish.items())))
        p("  end with d5 >= thres (no factor): %d = %.1f %% of the far queries" % (nofac, 100.0 * nofac / far))
        p("  rows of shells >= 2 per far query: in grid %.1f, visited as it stood %.1f (empty %.1f), with the gate's clip %.1f (empty %.1f)"
          % (rows_all / far, rows_now / far, empty_now / far, rows_clip / far, empty_clip / far))
        p("  of the rows visited as it stood: %.1f %% empty or outside the gate's sphere (%.1f %% outside, %.1f %% empty inside)"
          % (100.0 * (rows_now - rows_clip + empty_clip) / max(rows_now, 1), 100.0 * (rows_now - rows_clip) / max(rows_now, 1),
             100.0 * empty_clip / max(rows_now, 1)))
    return dict(n=n, far=far, rows_now=rows_now, rows_clip=rows_clip, empty_clip=empty_clip)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=8)
    ap.add_argument("--tiles", type=int, default=9, help="copies of the scene in the map (bench config 1 grows to 200 k points)")
    ap.add_argument("--thres", type=float, default=25.0)
    ap.add_argument("--cpu-extractor", default=None, metavar="DIR:MODULE", help="CPU restatement of the extraction (default: the product on device 0)")
    args = ap.parse_args()
    from scipy.spatial.transform import Rotation as Rsc
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    O = ctx = None
    if args.cpu_extractor:
        d, m = args.cpu_extractor.rsplit(":", 1)
        sys.path.insert(0, os.path.abspath(d))
        O = importlib.import_module(m)
        if hasattr(O, "build"):
            O.build()
    else:
        M = importlib.import_module("multi-modal-loam_amd")
        ctx = M.Context(max_scans=1)
    cfg = dict(n_rings=16, n_az=1800, pitch0=-15.0, pitch_step=2.0, livox=24000)  # bench.py CONFIGS[1]
    layout = dict(n_rings=cfg["n_rings"], pitch0=cfg["pitch0"], pitch_step=cfg["pitch_step"])
    leaf = (0.4, 0.2)
    base = 100

    def scan(k, motion):
        v = synth.velo_scan(k, n_rings=cfg["n_rings"], n_az=cfg["n_az"], pitch0=cfg["pitch0"], pitch_step=cfg["pitch_step"], motion=motion)
        l = synth.livox_scan(k, n=cfg["livox"], motion=motion)
        if ctx is not None:  # the product's path, as bench.py::build_maps drives it
            dR, dt = synth.sweep_motion(k) if motion else (np.eye(3), np.zeros(3))
            ctx.scan_upload(0, v, l)
            ctx.extract(0, 1)
            ctx.undistort(0, 1, np.asarray(dR).reshape(1, 9), np.asarray(dt).reshape(1, 3))
            ctx.downsample(0, 1)
            return ctx.features_download(0, 0), ctx.features_download(0, 1)
        ev, el = O.extract_velo(v, **layout), O.extract_livox(l)
        xyz = np.concatenate([ev["xyzi"][:, :3], el["xyzi"][:, :3]])
        lab = np.concatenate([ev["label"], el["label"]])
        rel = np.concatenate([ev["reltime"], el["reltime"]])
        if motion:
            dR, dt = synth.sweep_motion(k)
            xyz = O.undistort(xyz, rel, dR, dt)
        return O.voxel_downsample(xyz[lab == 1], leaf[0]), O.voxel_downsample(xyz[lab == 2], leaf[1])
    cm, sm = [], []
    for k in range(base - 8, base):
        c, s = scan(k, False)
        T = synth.pose_matrix(k)
        cm.append(synth.transform(T, c.astype(np.float64)).astype(F))
        sm.append(synth.transform(T, s.astype(np.float64)).astype(F))
    cm, sm = synth.voxel_filter(np.concatenate(cm), leaf[0]), synth.voxel_filter(np.concatenate(sm), leaf[1])
    maps = [synth.grow_map(cm, args.tiles * len(cm), seed=7), synth.grow_map(sm, args.tiles * len(sm), seed=8)]
    feats = [[], []]
    for k in range(base, base + args.scans):
        c, s = scan(k, True)
        Tp = synth.pose_matrix(k).copy()
        Tp[:3, 3] += np.array([0.03, -0.02, 0.01])
        Tp[:3, :3] = Tp[:3, :3] @ Rsc.from_rotvec([0.002, -0.001, 0.004]).as_matrix()
        feats[0].append(synth.transform(Tp, c.astype(np.float64)).astype(F))
        feats[1].append(synth.transform(Tp, s.astype(np.float64)).astype(F))
    out = sys.stdout
    print("far-query census: config 1, %d scans (k = %d..), map of %d tiles, thres_dist %g" % (args.scans, base, args.tiles, args.thres), file=out)
    tot = dict(n=0, far=0, rows_now=0, rows_clip=0, empty_clip=0)
    for kind, name in enumerate(("corner", "surf")):
        r = census_kind(name, np.concatenate(feats[kind]), maps[kind], 5.0 * leaf[kind], args.thres, out)
        for k in tot:
            tot[k] += r[k]
    print("both kinds: far %.2f %% of %d queries; rows visited per far query %.1f -> %.1f with the clip (%.1f %% fewer); "
          "%.1f %% of the rows visited as it stood are empty or outside the sphere"
          % (100.0 * tot["far"] / max(tot["n"], 1), tot["n"], tot["rows_now"] / max(tot["far"], 1), tot["rows_clip"] / max(tot["far"], 1),
             100.0 * (tot["rows_now"] - tot["rows_clip"]) / max(tot["rows_now"], 1),
             100.0 * (tot["rows_now"] - tot["rows_clip"] + tot["empty_clip"]) / max(tot["rows_now"], 1)), file=out)


if __name__ == "__main__":
    main()
