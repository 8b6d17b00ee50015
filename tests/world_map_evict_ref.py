"""A numpy restatement of the world map's eviction rule (csrc/world_map_evict.h, include/mmloam_hip.h "eviction") over whole
arrays, independent of the library; the host test holds the header's own program against it line by line, the GPU tests hold
mml_world_map_evict against it.

    goes         box test by mode -- OUTSIDE (0): not inside, INSIDE (1): inside, NOBOX (2): never -- OR count < min_count;
                 inside: lo[a] <= index[a] < hi[a] on all three axes (an empty box holds nothing)
    index box    index(v) = floor(float64(float32(v) * inv)) with inv = float32(1) / float32(leaf), the product in float32;
                 lo = index(lo_xyz), hi = index(hi_xyz) + 1, both clamped to [-2^17, 2^17]; None when a coordinate or the leaf
                 is not finite or the leaf is not positive
    evict        per named map: survivors = the export's rows that do not go, rows = those that do, both in the export's order
                 (ascending packed key: k, then j, then i); maps not named are returned as they are
"""
import numpy as np

HALF = 1 << 17
OUTSIDE, INSIDE, NOBOX = 0, 1, 2
F32 = np.float32


def rule(map, mode=NOBOX, lo=(0, 0, 0), hi=(0, 0, 0), min_count=0):
    return dict(map=int(map), mode=int(mode), lo=tuple(int(v) for v in lo), hi=tuple(int(v) for v in hi), min_count=int(min_count))


def inside(r, ijk):
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    lo, hi = np.asarray(r["lo"], np.int64), np.asarray(r["hi"], np.int64)
    return ((ijk >= lo) & (ijk < hi)).all(axis=1)


def goes(r, ijk, counts):
    """(n,) bool: which of the voxels ijk (n, 3) with the point counts (n,) the rule evicts"""
    ins = inside(r, ijk)
    box = ~ins if r["mode"] == OUTSIDE else ins if r["mode"] == INSIDE else np.zeros(len(ins), bool)
    return box | (np.asarray(counts, np.int64).reshape(-1) < r["min_count"])


def index_box(leaf, lo_xyz, hi_xyz):
    leaf = F32(leaf)
    lo_xyz, hi_xyz = np.asarray(lo_xyz, np.float32).reshape(3), np.asarray(hi_xyz, np.float32).reshape(3)
    if not (np.isfinite(leaf) and leaf > 0 and np.isfinite(lo_xyz).all() and np.isfinite(hi_xyz).all()):
        return None
    with np.errstate(all="ignore"):
        inv = F32(1.0) / leaf
        f_lo = np.floor((lo_xyz * inv).astype(np.float64))
        f_hi = np.floor((hi_xyz * inv).astype(np.float64)) + 1.0
    clamp = lambda f: np.where(f >= -HALF, np.minimum(f, HALF), -HALF).astype(np.int64)    # (a NaN product goes to the low end)
    return clamp(f_lo), clamp(f_hi)


def take(rows, sel):
    """The rows of an export dict (ijk, sums, counts, moments or None) chosen by the mask or index array `sel`"""
    return {k: (None if v is None else v[sel]) for k, v in rows.items()}


def evict(exports, rules):
    """exports: {map: export dict} of every map; rules: a list of rule().  Returns (survivors {map: dict}, evicted {map: dict} for
    the named maps, infos [dict(n_before, n_evicted, n_kept, first_row)] per rule)."""
    left, gone, infos = dict(exports), {}, []
    for r in rules:
        e = exports[r["map"]]
        g = goes(r, e["ijk"], e["counts"])
        left[r["map"]], gone[r["map"]] = take(e, ~g), take(e, g)
        infos.append(dict(n_before=len(g), n_evicted=int(g.sum()), n_kept=int((~g).sum())))
    for r, i in zip(rules, infos):
        i["first_row"] = sum(j["n_evicted"] for q, j in zip(rules, infos) if q["map"] < r["map"])
    return left, gone, infos


def same(a, b):
    """two export dicts, bit for bit"""
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and a[k].dtype == b[k].dtype and
                                                   a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes())
               for k in ("ijk", "sums", "counts", "moments"))
