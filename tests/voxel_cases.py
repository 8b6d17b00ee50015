"""Labelled clouds for the per-slot voxel filter (k_voxel of csrc/undistort_voxel.hip, the global-sort redo of csrc/map_upkeep.hip)
and a plain restatement of what it must compute.  numpy only: no oracle, no project header.

  voxel_ref(xyz, leaf)   pcl::VoxelGrid::applyFilter of PCL 1.8.1 (filters/impl/voxel_grid.hpp) on an n x 3 float32 cloud, with float32
                         scalars where PCL has floats: inverse leaf, getMinMax3D, min_b / div_b, the "integer indices would overflow"
                         return of the input, floor(p * inv) - float(min_b), i + j dx + k dx dy, a stable sort on the index, one
                         sequential float sum per voxel in input order, the division by float(count).
  records(...)           48-byte PointXYZINormal rows for Context.cloud_upload; the label rides in normal_z.
  Case                   one slot's cloud: a corner list and a surf list (each n x 3 float32 in FUSED order), label-0 filler, and where
                         the three are put.  Case.cloud() interleaves them; the relative order of a list's points is kept, so the
                         labelled points of kind k in fused order are Case.lists[k] itself.
  *_cases()              the tables the GPU tests walk (tests/test_gpu_voxel_forms.py); tests/test_voxel_cases.py asserts on the CPU
                         that every list has the count and the voxel structure its spec names.

A list is made from a spec (a dict).  Most specs put their points on a line along x, y and z inside one voxel: the voxel
index is then the voxel's ordinal on the line and a point's place in the sorted order is known by construction.  The line starts at
x = 40 m and the x of a voxel's points differ, so the order of the float32 sum changes the bits; the points of a list are shuffled, so
the fused order (= the order of the label list the kernel reads) is unrelated to the voxel order."""
import zlib

import numpy as np

LEAF = (0.4, 0.2)          # leaf_corner, leaf_surf (the context's defaults)
INT_MAX = 2147483647
F = np.float32
X0, Y0, Z0 = 40.0, 30.0, -20.0   # where the lines start (whole voxels at both leaves): a few points add up to hundreds of metres


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _grid(xyz, leaf):
    inv = F(1) / F(leaf)
    mn, mx = xyz.min(axis=0), xyz.max(axis=0)                     # float32
    min_b = np.floor(mn * inv).astype(np.int64)                   # static_cast<int>(floor(min_p[c] * inverse_leaf_size_[c]))
    max_b = np.floor(mx * inv).astype(np.int64)
    div_b = max_b - min_b + 1
    d = ((mx - mn) * inv).astype(np.int64) + 1                    # static_cast<int64_t>((max_p[c] - min_p[c]) * inv) + 1
    return inv, min_b, div_b, int(d[0]) * int(d[1]) * int(d[2]) > INT_MAX


def grid_overflows(xyz, leaf):
    """applyFilter's "Leaf size is too small for the input dataset" predicate"""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    return len(xyz) > 0 and _grid(xyz, leaf)[3]


def voxel_index(xyz, leaf):
    """centroid index of every point (unsigned 32 bits, as PCL's cloud_point_index_idx holds it)"""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    inv, min_b, div_b, _ = _grid(xyz, leaf)
    ijk = (np.floor(xyz * inv) - min_b.astype(F)).astype(np.int64)      # float32 subtraction, then static_cast<int>
    assert ijk.dtype == np.int64 and (np.floor(xyz * inv)).dtype == F
    mul1, mul2 = int(div_b[0]), int(div_b[0]) * int(div_b[1])
    return ((ijk[:, 0] + ijk[:, 1] * mul1 + ijk[:, 2] * mul2) & 0xffffffff).astype(np.uint32)   # int arithmetic, two's complement


def voxel_runs(xyz, leaf):
    """(order, starts, lengths): the stable ascending order on the voxel index and its runs of equal index"""
    idx = voxel_index(xyz, leaf)
    order = np.argsort(idx, kind="stable")
    s = idx[order]
    starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    return order, starts, np.diff(np.concatenate([starts, [len(s)]]))


def seq_sum(pts):
    """float32 sum of the rows in the order given, from 0.f (Eigen's Vector3f accumulator): np.cumsum adds one after the other"""
    return np.cumsum(np.concatenate([np.zeros((1, 3), F), pts]), axis=0, dtype=F)[-1]


def voxel_ref(xyz, leaf):
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    if len(xyz) == 0:
        return np.zeros((0, 3), F)
    if _grid(xyz, leaf)[3]:
        return xyz.copy()                                         # "output = *input"
    order, starts, lengths = voxel_runs(xyz, leaf)
    out = np.empty((len(starts), 3), F)
    single = lengths == 1
    out[single] = (np.zeros(3, F) + xyz[order[starts[single]]]) / F(1)
    for v in np.flatnonzero(~single):
        out[v] = seq_sum(xyz[order[starts[v]:starts[v] + lengths[v]]]) / F(lengths[v])
    assert out.dtype == F
    return out


# ---- records -----------------------------------------------------------------------------------------------------------------------
def records(xyz, label, n_velo, max_velo_points=None, full=False):
    """x y z _ | normal_x (in-sweep time) normal_y (line) normal_z (label) _ | intensity _ _ _.  The Velodyne part ends before the
    cloud and before the slot's Velodyne region does, so that a Livox point's storage position is not its fused index (`full`: the
    one cloud that fills its slot to the last place)."""
    n = len(xyz)
    if not full:
        assert 0 < n_velo < n and (max_velo_points is None or n_velo < max_velo_points)
    rec = np.zeros((n, 12), F)
    rec[:, :3] = xyz
    rec[:, 4] = 0.5
    rec[:, 5] = np.arange(n) % 6
    rec[:, 6] = label
    rec[:, 8] = 1 + np.arange(n) % 251
    return rec


# ---- lists -------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _line(lengths, leaf, rng, first_voxel=0):
    """voxel j of the line (j = first_voxel + its place in `lengths`) gets lengths[j] points with distinct x inside it"""
    lengths = np.asarray(lengths, np.int64)
    j = np.repeat(first_voxel + np.arange(len(lengths)), lengths)
    u = rng.uniform(0.15, 0.85, len(j))
    xyz = np.empty((len(j), 3), F)
    xyz[:, 0] = (X0 + (j + u) * leaf).astype(F)
    xyz[:, 1] = (Y0 + rng.uniform(0.15, 0.85, len(j)) * leaf).astype(F)    # (inside the one voxel that starts at Y0 / at Z0)
    xyz[:, 2] = (Z0 + rng.uniform(0.15, 0.85, len(j)) * leaf).astype(F)
    return xyz


def _mixed_lengths(n, rng):
    """run lengths 1..3 that add up to n"""
    out = []
    while n > 0:
        r = min(int(rng.integers(1, 4)), n)
        out.append(r)
        n -= r
    return out


def _ordinary(n, rng, leaf):
    """a room-sized cloud with a few points per voxel"""
    return rng.uniform(-3.0, 3.0, (n, 3)).astype(F) * F(leaf * 4)


def spec_n(spec):
    k = spec["kind"]
    if k == "edge":
        return spec["T"] - 1 + spec["r"] + spec["extra"]
    return spec["n"]


def spec_name(spec):
    k = spec["kind"]
    if k == "edge":
        return "edge%d_r%d_%d" % (spec["T"], spec["r"], spec["extra"])
    return "voxels%d_in_%d" % (spec["n"], spec["voxels"]) if k == "voxels" else "%s%d" % (k, spec["n"])


def make_list(spec, leaf):
    """the list's points in FUSED order (shuffled against the voxel order).  Where the spec is about the order of a voxel's sum, every
    voxel of three or more points gives other bits when it is summed backwards (the next seed is taken until that holds)."""
    for attempt in range(16):
        pts = _make_list(spec, leaf, attempt)
        if spec["kind"] not in ("edge", "one", "digit16") or len(pts) < 3:
            return pts
        order, starts, lengths = voxel_runs(pts, leaf)
        if all(seq_sum(pts[order[s:s + m]]).tobytes() != seq_sum(pts[order[s:s + m]][::-1]).tobytes() for s, m in zip(starts, lengths) if m >= 3):
            return pts
    raise AssertionError(spec)


def _make_list(spec, leaf, attempt):
    kind, n = spec["kind"], spec_n(spec)
    rng = _rng(spec_name(spec), leaf, attempt)
    if n == 0:
        return np.zeros((0, 3), F)
    if kind == "count":
        xyz = _line(_mixed_lengths(n, rng), leaf, rng)
    elif kind == "own":
        xyz = _line([1] * n, leaf, rng)
    elif kind == "one":
        xyz = _line([n], leaf, rng)
    elif kind == "voxels":                     # n points in exactly spec["voxels"] voxels
        v = spec["voxels"]
        lengths = np.ones(v, np.int64)
        np.add.at(lengths, rng.integers(0, v, n - v), 1)
        xyz = _line(lengths, leaf, rng)
    elif kind == "edge":
        xyz = _line([1] * (spec["T"] - 1) + [spec["r"]] + [1] * spec["extra"], leaf, rng)
    elif kind == "digit16":                    # two voxels, 65536 apart: the index's two low digits agree on every key
        a = n // 2
        xyz = np.concatenate([_line([a], leaf, rng), _line([n - a], leaf, rng, first_voxel=65536)])
    elif kind == "digit24":                    # a thin box of 32768 x 256 x 255 voxels (just below 2^31), the points all over it
        dims = np.array([32768, 256, 255])
        ijk = np.stack([rng.integers(0, d, n) for d in dims], axis=1)
        ijk[0] = 0
        ijk[1] = dims - 1
        ijk[2:n // 2] = ijk[n // 2:n // 2 + n // 2 - 2]            # every other voxel holds two points
        u = rng.uniform(0.3, 0.7, (n, 3))
        u[:2] = 0.5
        xyz = ((ijk + u) * leaf).astype(F)
    elif kind == "overflow":                   # two points 1e4 m apart on every axis: more than INT_MAX voxels in the box
        xyz = _ordinary(n, rng, leaf)
        xyz[0] = (-5000.0, -5000.0, -5000.0)
        xyz[1] = (5000.0, 5000.0, 5000.0)
    elif kind == "arith":                      # coordinates exactly k * leaf as float32, both signs, -0.0, exact duplicates
        k = rng.integers(-12, 13, (n, 3))
        xyz = k.astype(F) * F(leaf)
        q = n // 4
        xyz[q:2 * q] = rng.uniform(-2.0, 2.0, (q, 3)).astype(F)    # ordinary negative and positive coordinates among them
        xyz[2 * q:3 * q] = xyz[:q]                                 # duplicates of the lattice points
        xyz[3 * q:3 * q + 8] = xyz[q:q + 8]                        # ... and of ordinary ones
        xyz[3 * q + 8:3 * q + 16] = np.where(k[:8] % 2 == 0, F(-0.0), F(0.0))
        xyz[3 * q + 16:3 * q + 20, 0] = F(-0.0)
    else:
        raise ValueError(kind)
    assert xyz.dtype == F and len(xyz) == n
    return xyz[rng.permutation(n)]


def count(n):
    return dict(kind="count", n=n)


def own(n):
    return dict(kind="own", n=n)


def one(n):
    return dict(kind="one", n=n)


def edge(T, r, extra=5):
    return dict(kind="edge", T=T, r=r, extra=extra)


def other(kind, n, **kw):
    return dict(kind=kind, n=n, **kw)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class Case:
    """layout "mixed": label-0, label-1 and label-2 points interleaved at random over the whole cloud of n points.
    layout "tail": `fill` label-0 points first, then the labelled ones interleaved: they hold the cloud's highest fused indices."""

    def __init__(self, name, corner, surf, n=None, fill=64, n_livox=37, layout="mixed", full=False):
        self.name, self.specs, self.layout, self.full = name, (corner, surf), layout, full
        self.counts = (spec_n(corner), spec_n(surf))
        self.n = n if n is not None else sum(self.counts) + fill
        assert self.n >= sum(self.counts)
        self.n_velo = self.n - n_livox
        self._lists = None

    @property
    def lists(self):
        if self._lists is None:
            self._lists = tuple(make_list(s, LEAF[k]) for k, s in enumerate(self.specs))
        return self._lists

    def cloud(self):
        """(xyz, label) of the fused cloud"""
        rng = _rng("cloud", self.name)
        nc, ns = self.counts
        label = np.zeros(self.n, np.int32)
        if self.layout == "mixed":
            where = rng.permutation(self.n)[:nc + ns]
        else:
            where = self.n - (nc + ns) + rng.permutation(nc + ns)
        label[where[:nc]] = 1
        label[where[nc:]] = 2
        xyz = rng.uniform(-60.0, 60.0, (self.n, 3)).astype(F)
        xyz[label == 1] = self.lists[0]            # (ascending positions: the list's own order is the fused order)
        xyz[label == 2] = self.lists[1]
        return xyz, label

    def records(self, max_velo_points=None):
        xyz, label = self.cloud()
        return records(xyz, label, self.n_velo, max_velo_points, self.full)

    def expected(self, kind):
        key = (spec_name(self.specs[kind]), kind)
        if key not in _REF:
            _REF[key] = voxel_ref(self.lists[kind], LEAF[kind])
            _REF[key].setflags(write=False)
        return _REF[key]


_REF = {}   # one reference per (list, leaf), shared by every test that needs it


def pair(prefix, corner_specs, surf_specs, cap, **kw):
    """Short corner lists with long surf lists: every cloud fits `cap` points.  The shorter table is filled up with 7-point lists."""
    cs = sorted(corner_specs, key=spec_n)
    ss = sorted(surf_specs, key=spec_n, reverse=True)
    m = max(len(cs), len(ss))
    cs = cs + [count(7)] * (m - len(cs))
    ss = ss + [count(7)] * (m - len(ss))
    out = []
    for c, s in zip(cs, ss):
        fill = min(64, cap - spec_n(c) - spec_n(s))
        assert fill >= 0, (spec_name(c), spec_name(s))
        out.append(Case("%s:%s+%s" % (prefix, spec_name(c), spec_name(s)), c, s, fill=max(fill, 38 - spec_n(c) - spec_n(s)), **kw))
    return out


SMALL_COUNTS = [0, 1, 2, 63, 64, 65]
CAP = 9000 + 37 - 1      # points of a cloud for a context of 9000 Velodyne + 600 Livox points: n_velo < 9000, 37 Livox points


def small_batch_cases():
    """calls of at most 16 slots: both kinds on the 1024-thread form (corner capacity 2048, surf 8192)"""
    corner = [count(n) for n in SMALL_COUNTS + [1023, 1024, 1025, 2047, 2048]]
    corner += [edge(1024, r) for r in (2, 64, 65, 66)]          # (r = T + 70 does not fit the corner capacity)
    corner += [one(300), one(2048), own(2048), own(257), other("digit16", 600), other("digit24", 500), other("arith", 400),
               other("overflow", 300), other("overflow", 2049), count(2049)]
    surf = [count(n) for n in SMALL_COUNTS + [2049, 4096, 4097, 8192]]
    surf += [edge(1024, r) for r in (2, 64, 65, 66, 1024 + 70)]
    surf += [one(1), one(300), one(2048), own(4097), own(1000), other("digit16", 600), other("digit24", 3000), other("arith", 400),
             other("overflow", 300), other("overflow", 8193), count(8193)]
    return pair("small", corner, surf, CAP)


def large_batch_cases():
    """calls of more than 16 slots: 256-thread corners (2048), 512-thread surf (4096), the listed 1024-thread form (8192)"""
    corner = [count(n) for n in SMALL_COUNTS + [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]]
    corner += [edge(256, r) for r in (2, 64, 65, 66, 256 + 70)]
    corner += [one(300), one(2048), own(2048), other("digit16", 600), other("digit24", 500), other("arith", 400),
               other("overflow", 300), other("overflow", 2049), count(2049)]
    surf = [count(n) for n in SMALL_COUNTS + [511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192]]
    surf += [edge(512, r) for r in (2, 64, 65, 66, 512 + 70)]
    surf += [one(300), one(2048), own(4096), other("digit16", 600), other("digit24", 3000), other("arith", 400),
             other("overflow", 300), other("overflow", 8193), count(8193), edge(1024, 1024 + 70)]
    return pair("large", corner, surf, CAP)


def independence_cases():
    """23 clouds for slots 0 .. 22: short and long lists of every form, big surf lists (listed form, redo) from slot 3 on"""
    corner = [count(n) for n in (0, 1, 65, 255, 256, 257, 513, 1024, 1025, 2047, 2048, 2049)] + [edge(256, 66), edge(256, 326), one(300)]
    corner += [count(n) for n in (100, 200, 300, 400, 500, 600, 700, 800)]
    surf = [count(n) for n in (0, 1, 65, 511, 512, 513, 1025, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)]
    surf += [edge(512, 66), edge(512, 582), one(2048), own(4097)] + [count(n) for n in (3000, 3100, 3200, 3300)]
    cases = pair("indep", corner, surf, CAP)
    assert len(cases) == 23
    # (pair() sorts the surf lists longest first: put the five longest at slots 3, 7, 11, 15, 19 instead of 0 .. 4)
    order = list(range(5, 23))
    for k, at in enumerate((3, 7, 11, 15, 19)):
        order.insert(at, k)
    return [cases[i] for i in order]


def quiet_cases(n):
    """clouds without a list beyond any form's capacity"""
    return [Case("quiet%d" % i, count(40 + 90 * i), count(300 + 180 * i)) for i in range(n)]


def long_list_cases():
    """four distinct clouds with 4097 surf points and four small ones (test_listed_form_longer_than_its_grid cycles them over 300 slots)"""
    big = [Case("listed%d" % i, count(3 + 50 * i), s, fill=16, n_livox=11)
           for i, s in enumerate((count(4097), own(4097), dict(kind="voxels", n=4097, voxels=900), edge(1024, 1094, extra=4097 - 1023 - 1094)))]
    small = [Case("listed_small%d" % i, count(10 + 100 * i), count(100 + 1200 * i), fill=16, n_livox=11) for i in range(4)]
    return big, small


WIDE_N, WIDE_LIVOX = 65650, 60


def wide_cases():
    """65650-point clouds for a context of 65600 + 64 points (NT > 65536: the wide key layout, the 8192-key form for both kinds); the
    labelled points are the cloud's last ones"""
    kw = dict(n=WIDE_N, n_livox=WIDE_LIVOX, layout="tail")
    return [Case("wide:8191+8192", count(8191), count(8192), **kw),
            Case("wide:8192+8191", own(8192), count(8191), **kw),
            Case("wide:8193+small", count(8193), count(65), **kw),
            Case("wide:small+8193", count(1), count(8193), **kw),
            Case("wide:edges", edge(1024, 1094), edge(1024, 65), **kw),
            Case("wide:edges2", edge(1024, 66), edge(1024, 64), **kw),
            Case("wide:overflow", other("overflow", 300), other("overflow", 8193), **kw),
            Case("wide:digits", other("digit24", 500), other("digit16", 600), **kw)]


def full_cases():
    """2^20-point clouds that fill a slot of (2^20 - 64) + 64 points: the last labelled point has fused index 2^20 - 1"""
    kw = dict(n=1 << 20, n_livox=64, layout="tail", full=True)
    return [Case("full:2048+8192", count(2048), count(8192), **kw), Case("full:300+8193", one(300), count(8193), **kw)]


def capacity_cases():
    """for a context of max_features = 1000: as many voxels as fit and one more, on the LDS path and (2049 corners) the redo path"""
    v = lambda n, k: dict(kind="voxels", n=n, voxels=k)
    return [Case("cap:own1000", own(1000), own(1000)), Case("cap:own1001", own(1001), count(500)),
            Case("cap:redo1000", v(2049, 1000), v(3000, 1000)), Case("cap:redo1001", v(2049, 1001), v(3000, 1001))]


def all_cases():
    """every case of every table, once"""
    big, small = long_list_cases()
    seen, out = set(), []
    for c in (small_batch_cases() + large_batch_cases() + independence_cases() + quiet_cases(20) + big + small + wide_cases() + full_cases()
              + capacity_cases()):
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)
    return out
