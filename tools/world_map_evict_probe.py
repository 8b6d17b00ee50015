#!/usr/bin/env python3
"""Eviction from the world map two ways, alternated in one run -> profiles/world_map_evict_probe.txt

    python tools/world_map_evict_probe.py [--out profiles/world_map_evict_probe.txt] [--reps 5]

Tables of 2^12, 2^16 and 2^20 positions about a quarter full (two plain maps of equal size, hand-made rows through
world_map_import); 1 %, 50 % and 100 % of map 0 go, chosen by an index box along i.  The ways:

    host    what the parent commit offers: world_map_export(0), a numpy filter, world_map_reset(0), world_map_import of the survivors
    evict   one mml_world_map_evict with the rows handed back (Context.world_map_evict: a dry run for the size, then the call)
    drop    one mml_world_map_evict, rows dropped

Before every timed call the map is restored (reset + import of the original rows, not timed); after it both maps are exported
and compared bitwise with the numpy filter of the original.  Times are wall clock around the calls, median and range over the
repetitions; bytes over the link are what the calls copy by their definition.  One run: nothing is gated on it and no speed-up
is to be claimed from it."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEAF = 0.25


def make_rows(rng, n, span):
    """n voxels in export order; every voxel has an i of its own, so that a box along i cuts off any share exactly"""
    ijk = np.stack([rng.permutation(n) - n // 2, rng.integers(-span, span, n), rng.integers(-span, span, n)], 1).astype(np.int32)
    ijk = ijk[np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))]
    return dict(ijk=np.ascontiguousarray(ijk), sums=rng.normal(0, 50, (n, 4)).astype(np.float32), counts=rng.integers(1, 10, n).astype(np.int32), moments=None)


def take(rows, sel):
    return {k: (None if v is None else v[sel]) for k, v in rows.items()}


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("ijk", "sums", "counts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_map_evict_probe.txt"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    M = importlib.import_module("multi-modal-loam_amd")
    rng = np.random.default_rng(3)
    lines = ["world_map_evict_probe: eviction of part of map 0 of two plain maps, three ways alternated, %d repetitions each" % args.reps,
             "ms: median (min .. max) of the wall clock around the calls; KiB: bytes over the link, down + up; one run, nothing gated", ""]
    ok = True
    for bits in (12, 16, 20):
        slots = 1 << bits
        capacity, n = slots // 2, slots // 8                       # two maps of slots / 8 voxels: a quarter of the positions
        span = 64
        rows = [make_rows(rng, n, span), make_rows(rng, n, span)]
        c = M.Context(max_scans=1, max_velo_points=1024, max_livox_points=1024)
        try:
            c.world_map_create(2, LEAF, capacity)
            c.world_map_import(1, **rows[1])
            for share in (0.01, 0.5, 1.0):
                cut = n if share == 1.0 else int(share * n) - n // 2        # i < cut: exactly int(share n) voxels
                goes = rows[0]["ijk"][:, 0] < cut                    # INSIDE the box i < cut
                left, gone = take(rows[0], ~goes), take(rows[0], goes)
                rule = M.wm_evict_rule(0, M.WM_EVICT_INSIDE, (-n, -span, -span), (cut, span, span))
                row_bytes = 12 + 16 + 4
                t = {"host": [], "evict": [], "drop": []}
                for rep in range(args.reps):
                    for way in ("host", "evict", "drop"):
                        c.world_map_reset(0)
                        c.world_map_import(0, **rows[0])
                        c.synchronize()
                        t0 = time.perf_counter()
                        if way == "host":
                            e = c.world_map_export(0)
                            keep = ~(e["ijk"][:, 0] < cut)
                            back = take(e, ~keep)
                            c.world_map_reset(0)
                            c.world_map_import(0, **take(e, keep))
                        elif way == "evict":
                            back = c.world_map_evict([rule])[1][0]
                        else:
                            c.world_map_evict([rule], rows=False)
                            back = gone
                        c.synchronize()
                        t[way].append((time.perf_counter() - t0) * 1e3)
                        good = same(c.world_map_export(0), left) and same(c.world_map_export(1), rows[1]) and same(back, gone) and \
                            c.world_map_size(0) == len(left["ijk"]) and c.world_map_size(-1) == len(left["ijk"]) + n
                        ok = ok and good
                        if not good:
                            lines.append("MISMATCH: 2^%d positions, %.0f %%, %s, repetition %d" % (bits, 100 * share, way, rep))
                link = {"host": row_bytes * (n + len(left["ijk"])), "evict": row_bytes * len(gone["ijk"]), "drop": 0}
                for way in ("host", "evict", "drop"):
                    v = np.array(t[way])
                    lines.append("2^%-2d positions  %7d voxels in map 0  %5.1f %% evicted (%7d)  %-5s  %9.3f ms (%9.3f .. %9.3f)  %10.1f KiB" % (
                        bits, n, 100.0 * len(gone["ijk"]) / n, len(gone["ijk"]), way, np.median(v), v.min(), v.max(), link[way] / 1024.0))
                lines.append("")
        finally:
            c.close()
    lines.append("every final export, handed-back row set and size compared bitwise with the numpy filter: %s" % ("all equal" if ok else "MISMATCH"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
