"""Hand-built increment histories for the local-map increment chain (csrc/map_upkeep.hip: k_inc_to_world, k_inc_concat_bbox,
k_inc_voxel_keys, the sort, heads and scan, k_inc_centroid, k_inc_bbox_out): the ring, voxel and count edges that scene-shaped data
does not reach.  tests/test_local_map_cases_census.py checks on the oracle alone that every case is what its name claims;
tests/test_gpu_local_map_edges.py runs them on the device against O.LocalMap.

A case is a plain dict:
  name, family ("A" .. "E"),
  incs = [(corner stack, surf stack, 4 x 4 pose)], float32 stacks of at most MAX_FEATURES rows, the two kinds of different sizes,
  check_from = the first increment after which the maps are compared,
  refused = the increments the library must refuse (family E; the oracle never sees them),
  max_map_points (family E), knn_at = the increment after which the rebuilt grid is queried (or absent),
  expect = what the census asserts, per family.
A bank case (family F) is a dict: name, banks = [content name per bank of the call], calls = [[(corner, surf, pose) per bank]],
big = the position of the 65 537-point bank or None.

Builders take the oracle module O where a case has to be found by asking it (family D)."""
import numpy as np

F32 = np.float32
WINDOW = 50            # localMapWindowSize
MAX_FEATURES = 8192    # the default max_features: rows of a stack
LEAF = (0.4, 0.2)      # the default leaf_corner, leaf_surf
EMPTY = np.zeros((0, 3), F32)
EYE = np.eye(4)
RUNS = (1, 2, 63, 64, 65)   # points per voxel of the mixed clouds: either side of a wavefront


def pose(angle_deg=0.0, t=(0.0, 0.0, 0.0), axis=(0.0, 0.0, 1.0)):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def to_world(T, xyz):
    """pointAssociateToMap as the oracle and k_inc_to_world write it: double products summed left to right, one cast to float."""
    p, T = np.asarray(xyz, F32).reshape(-1, 3).astype(np.float64), np.asarray(T, np.float64)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1).astype(F32)


def voxel_of(world, leaf):
    """floor(x * (1 / leaf)) in float, per axis: PCL's absolute voxel coordinate (the census checks it against the oracle)."""
    return np.floor(np.asarray(world, F32) * (F32(1.0) / F32(leaf))).astype(np.int64)


def _case(name, family, incs, check_from=0, **more):
    for c, s, T in incs:
        assert c.dtype == F32 and s.dtype == F32 and len(c) <= MAX_FEATURES and len(s) <= MAX_FEATURES, name
        assert np.isfinite(c).all() and np.isfinite(s).all() and np.asarray(T).shape == (4, 4), name
    return dict(name=name, family=family, incs=incs, check_from=check_from, refused=(), **more)


def _split(pts, sizes):
    assert sum(sizes) == len(pts)
    cut = np.cumsum([0] + list(sizes))
    return [pts[cut[i]:cut[i + 1]] for i in range(len(sizes))]


def ring_totals(case):
    """[increment] -> ((corner total, surf total), (empty corner slots, empty surf slots)) by the ring's definition alone."""
    n = np.zeros((2, WINDOW), int)
    out, k = [], 0
    for i, (c, s, _) in enumerate(case["incs"]):
        if i not in case["refused"]:
            n[0, k % WINDOW], n[1, k % WINDOW] = len(c), len(s)
            k += 1
        out.append(((int(n[0].sum()), int(n[1].sum())), tuple(tuple(np.flatnonzero(n[j] == 0)) for j in range(2))))
    return out


def oracle_history(O, case, leaf=LEAF):
    """[increment] -> (corner map, surf map) of one O.LocalMap fed the case; a refused increment repeats the maps before it."""
    lm = O.LocalMap(window=WINDOW, leaf_corner=leaf[0], leaf_surf=leaf[1])
    out = []
    for i, (c, s, T) in enumerate(case["incs"]):
        if i in case["refused"]:
            out.append(out[-1])
            continue
        lm.increment(c, s, T)
        out.append((lm.get(0), lm.get(1)))
    return out


# ---- clouds ---------------------------------------------------------------------------------------------------------------------

def lattice(n, leaf, seed, origin=(0.0, 0.0, 0.0)):
    """n points, each in a voxel of its own: (1.5 i + 0.25 .. 0.45) leaf on a cubic lattice, in shuffled order (the sorted order differs
    from the ring's)."""
    side = 1
    while side ** 3 < n:
        side += 1
    g = np.arange(side)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:n]
    rng = np.random.default_rng(seed)
    pts = ((1.5 * ijk + 0.25 + 0.2 * rng.uniform(0, 1, (n, 3))) * leaf + np.asarray(origin)).astype(F32)   # (jitter: no equal distances)
    return pts[rng.permutation(n)]


def one_voxel(n, leaf, seed, cell=(7, -3, 2)):
    """n points of ONE voxel with non-dyadic coordinates: their float sum depends on the order."""
    u = np.random.default_rng(seed).uniform(0.05, 0.95, (n, 3))
    return ((np.asarray(cell) + u) * leaf).astype(F32)


def mixed(n, leaf, seed):
    """n points in voxels of 1, 2, 63, 64, 65, 1, ... points (the last one cut short), shuffled.  Returns (points, voxels)."""
    counts = []
    while sum(counts) < n:
        counts.append(min(RUNS[len(counts) % len(RUNS)], n - sum(counts)))
    side = 1
    while side ** 3 < len(counts):
        side += 1
    g = np.arange(side)
    ijk = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[:len(counts)]
    rng = np.random.default_rng(seed)
    pts = np.concatenate([(2.0 * ijk[v] - 3.0 + 0.1 + 0.8 * rng.uniform(0, 1, (c, 3))) * leaf for v, c in enumerate(counts)]).astype(F32)
    return pts[rng.permutation(n)], len(counts)


def knn_queries(cloud, seed, n=64):
    """About n queries for a map: inside its box, on the box faces, outside it.  The check compares indices, so a query is kept
    only if its six nearest map points lie at clearly distinct distances (gaps above 2e-6 of the squared distance, some twenty
    float steps): candidates are drawn until every group is full."""
    rng = np.random.default_rng(seed)
    pts = cloud.astype(np.float64)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    ext = np.maximum(hi - lo, 1.0)

    def draw(group):
        q = rng.uniform(lo, lo + ext)
        if group == 1:
            a = int(rng.integers(0, 3))
            q[a] = (lo, hi)[int(rng.integers(0, 2))][a]
        if group == 2:
            q = lo + ext / 2 + rng.choice([-1.0, 1.0], 3) * rng.uniform(1.0, 4.0, 3) * ext
        return q.astype(F32)

    out = []
    for group, want in enumerate((n * 3 // 8, n * 3 // 8, n // 4)):
        kept = tries = 0
        while kept < want:
            q, tries = draw(group), tries + 1
            assert tries < 40 * want, "no tie-free queries for this map"
            d2 = np.sort(((pts - q.astype(np.float64)) ** 2).sum(axis=1))[:6]
            if len(d2) < 6 or (np.diff(d2) > 2e-6 * d2[1:]).all():
                out.append(q)
                kept += 1
    return np.array(out, F32)


# ---- A: ring occupancy -----------------------------------------------------------------------------------------------------------

def _ring_case(name, sizes_c, sizes_s, seed, check_from):
    rng = np.random.default_rng(seed)
    incs = []
    for i, (a, b) in enumerate(zip(sizes_c, sizes_s)):
        T = pose(3.0 * i, (0.37 * i, -0.21 * i, 0.05 * i))
        incs.append((rng.uniform(-5, 5, (a, 3)).astype(F32), rng.uniform(-5, 5, (b, 3)).astype(F32), T))
    return _case(name, "A", incs, check_from, expect=dict(sizes=(list(sizes_c), list(sizes_s))))


def cases_A():
    rng = np.random.default_rng(11)
    ii = [0, 0, 3, 0, 1, 0, 0, 257, 0]
    fifty_c, fifty_s = list(rng.integers(1, 4, WINDOW)), list(rng.integers(1, 4, WINDOW))
    return [
        # (i) both stacks empty, again, then points
        _ring_case("A.i.empty-first", [0, 0, 2, 1, 0], [0, 0, 3, 0, 2], 1, 0),
        # (ii) runs of empty slots between slots with points, one kind the mirror of the other
        _ring_case("A.ii.runs", ii, ii[::-1], 2, 0),
        # (iii) a full ring, then the wrap takes the points of slots 0 and 2 (corner) / 1 and 3 (surf): the ring starts empty
        _ring_case("A.iii.wrap-empties", fifty_c + [0, 2, 0, 1], fifty_s + [1, 0, 3, 0], 3, WINDOW),
        # (iv) 49 leading empty slots, slot 49 alone, then the wrap writes slot 0 and an empty slot 1
        _ring_case("A.iv.last-slot", [0] * 49 + [3, 2, 0], [0] * 49 + [1, 3, 0], 4, 0),
    ]


# ---- B: count edges --------------------------------------------------------------------------------------------------------------

B_SIZES = {1: [1], 2: [1, 1], 255: [128, 127], 256: [128, 128], 257: [256, 1], 65535: [MAX_FEATURES] * 7 + [MAX_FEATURES - 1],
           65536: [MAX_FEATURES] * 8, 65537: [MAX_FEATURES] * 8 + [1]}


def cases_B():
    out = []
    for n, sizes in B_SIZES.items():
        # corner: every point its own voxel; surf: all in one voxel, the stacks in reverse order (other sizes per increment)
        # (corner full one increment before surf: an empty stack opposite a large one at both ends)
        c, s = _split(lattice(n, LEAF[0], n), sizes) + [EMPTY], [EMPTY] + _split(one_voxel(n, LEAF[1], n + 1), sizes[::-1])
        out.append(_case("B.%d" % n, "B", [(a, b, EYE) for a, b in zip(c, s)], max(0, len(sizes) - 3), knn_at=len(sizes),
                         expect=dict(total=(n, n), filtered=(n, 1))))
    for n in (257, 65537):
        sizes = B_SIZES[n]
        m, nvox = mixed(n, LEAF[0], n + 2)
        c, s = _split(m, sizes) + [EMPTY], [EMPTY] + _split(lattice(n, LEAF[1], n + 3, origin=(-4.0, 2.0, 1.0)), sizes[::-1])
        out.append(_case("B.%d.mixed" % n, "B", [(a, b, EYE) for a, b in zip(c, s)], max(0, len(sizes) - 3), knn_at=len(sizes),
                         expect=dict(total=(n, n), filtered=(nvox, n))))
    return out


# ---- C: voxel edges --------------------------------------------------------------------------------------------------------------

C_POSES = {"identity": EYE,
           "far": pose(30.0, (1.0e4, -1.0e4, 50.0), axis=(1.0, 2.0, 3.0)),       # |t| = 1e4: the cast to float rounds at 1e-3
           "negative": pose(7.0, (-480.3, -490.7, -470.1), axis=(3.0, 1.0, 2.0))}   # the whole cloud below zero on every axis
C_K = (-3, -1, 0, 1, 2, 1000)


def edge_values(leaf):
    """k * leaf in float for k in C_K with its two float neighbours, and three x below k * leaf whose float product x * (1 / leaf)
    rounds up onto the integer k."""
    lf = F32(leaf)
    inv = F32(1.0) / lf
    vals = []
    for k in C_K:
        v = F32(k) * lf
        vals += [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]
    below = []
    for k in range(1, 4000):
        x = F32(k) * lf
        for _ in range(4):
            x = np.nextafter(x, F32(-np.inf))
            if F32(x * inv) == F32(k) and np.float64(x) * np.float64(inv) < k:
                below.append(x)
                break
        if len(below) == 3:
            break
    assert len(below) == 3, leaf
    return np.array(vals, F32), np.array(below, F32)


def edge_cloud(leaf):
    """Every edge value on every axis (the other two coordinates inside a voxel), on the diagonal without k = 1000, and a line."""
    vals, below = edge_values(leaf)
    allv = np.concatenate([vals, below])
    base = np.array([5.37, 6.41, 7.29]) * leaf
    pts = []
    for a in range(3):
        for v in allv:
            p = base.astype(F32)
            p[a] = v
            pts.append(p)
    diag = np.concatenate([vals[:3 * (len(C_K) - 1)], below])
    pts += [np.array([v, v, v], F32) for v in diag]
    # a skew line at steps below a leaf: which neighbours share a voxel depends on where the pose puts the voxel faces
    pts += [(base + 0.45 * leaf * j * np.array([1.0, 0.9, 0.8])).astype(F32) for j in range(1, 11)]
    return np.array(pts, F32)


def _robust_pairs(T, leaf):
    """Four features whose world images are a pair 0.2 leaf apart inside one voxel and a pair 0.2 leaf apart across a voxel face."""
    w0 = to_world(T, np.array([[10.3, 11.1, 9.7]]) * leaf)[0].astype(np.float64)
    v = np.floor(w0 / leaf)
    centre = (v + 0.5) * leaf
    face = np.array([v[0], v[1] + 3.0, v[2]]) * leaf + np.array([0.0, 0.5, 0.5]) * leaf
    d = np.array([0.1 * leaf, 0.0, 0.0])
    world = np.array([centre - d, centre + d, face - d, face + d])
    Ti = np.linalg.inv(np.asarray(T, np.float64))
    return (world @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32)


def cases_C():
    out = []
    for pname, T in C_POSES.items():
        stacks, expect = [], dict(merged=[], split=[], common=[])
        for kind, leaf in enumerate(LEAF):
            common = edge_cloud(leaf)
            if kind == 1:
                common = common[::-1].copy()                       # (the other kind in the other order)
            else:
                common = np.concatenate([common, lattice(7, leaf, 5, origin=(1.0, 1.0, 1.0))])   # (and of another size)
            pts = np.concatenate([common, _robust_pairs(T, leaf)])
            n = len(common)
            merged, split = [(n, n + 1)], [(n + 2, n + 3)]
            if pname == "identity":                                 # the float neighbours of k * leaf, as the voxel arithmetic sees them
                vox = voxel_of(to_world(T, pts), leaf)
                order = np.arange(n) if kind == 0 else np.arange(n)[::-1]
                for j in range(3 * len(C_K) - 1):                   # axis x block: values in ascending float order within a k
                    if j % 3 == 2:
                        continue
                    a, b = int(order[j]), int(order[j + 1])
                    (merged if (vox[a] == vox[b]).all() else split).append((a, b))
            stacks.append(pts)
            expect["merged"].append(merged)
            expect["split"].append(split)
            expect["common"].append(n)
        out.append(_case("C." + pname, "C", [(stacks[0], stacks[1], T)], 0, expect=expect))
    return out


# ---- D: the voxel index overflow -------------------------------------------------------------------------------------------------

def _dup_cloud(n, leaf, seed):
    """n points in [2, 6]^3 (in leaves: a few voxels a side), half of them a hundredth of a leaf from another one; shuffled."""
    rng = np.random.default_rng(seed)
    a = (2.0 + rng.uniform(0.05, 0.95, (n - n // 2, 3)) + rng.integers(0, 4, (n - n // 2, 3))) * leaf
    b = a[:n // 2] + 0.01 * leaf
    return np.concatenate([a, b])[rng.permutation(n)].astype(F32)


def overflow_extent(O, cloud, leaf):
    """(below, above): adjacent floats e such that the cloud plus the far points (0, 0, 0) and (e, e, e) is filtered / comes back
    as it went in -- found by asking the oracle's filter, bisecting on the float's bit pattern."""
    def unfiltered(bits):
        e = np.array([bits], np.int32).view(F32)[0]
        pts = np.concatenate([[[0, 0, 0]], [[e, e, e]], cloud]).astype(F32)
        return len(O.voxel_downsample(pts, leaf)) == len(pts)
    lo, hi = (int(np.array([F32(k * leaf)], F32).view(np.int32)[0]) for k in (1200, 1400))
    assert not unfiltered(lo) and unfiltered(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if unfiltered(mid):
            hi = mid
        else:
            lo = mid
    return tuple(np.array([b], np.int32).view(F32)[0] for b in (lo, hi))


def cases_D(O):
    clouds = [_dup_cloud(300, LEAF[0], 21), _dup_cloud(200, LEAF[1], 22)]
    ext = [overflow_extent(O, clouds[k], LEAF[k]) for k in range(2)]
    out = []
    for side, name in enumerate(("below", "above")):
        far = [np.array([[0, 0, 0], [ext[k][side]] * 3], F32) for k in range(2)]
        near = [(np.array([[1.1, 1.2, 1.3], [1.15, 1.2, 1.3], [3.3, 0.7, 2.9]]) * 2.0 * LEAF[k]).astype(F32) for k in range(2)]
        # slot 0: the far points; slot 1: the cloud; 48 empty slots; then the wrap replaces slot 0 and the ring filters normally
        incs = [(far[0], far[1], EYE), (clouds[0], clouds[1], EYE)] + [(EMPTY, EMPTY, EYE)] * (WINDOW - 2) + [(near[0], near[1][:2], EYE)]
        out.append(_case("D." + name, "D", incs, 0, knn_at=1, expect=dict(side=name, extent=[float(e[side]) for e in ext])))
    return out


# ---- E: capacity -----------------------------------------------------------------------------------------------------------------

E_MAX_MAP_POINTS = 300   # no lower limit is enforced by the context; a few hundred keeps every launch to two workgroups


def case_E():
    mm = E_MAX_MAP_POINTS
    c = lattice(mm + 1, LEAF[0], 31)
    s = lattice(mm + 1, LEAF[1], 32, origin=(3.0, -2.0, 0.5))
    incs = [(c[0:100], s[0:50], EYE), (c[100:200], s[50:70], EYE), (c[200:300], s[70:100], EYE),   # corner ring = max_map_points
            (c[300:301], s[100:105], EYE),                                                         # refused: corner 301
            (EMPTY, s[100:107], EYE),                                                              # slot 3
            (EMPTY, s[107:301], EYE),                                                              # refused: surf 107 + 194 = 301
            (EMPTY, s[107:300], EYE)]                                                              # slot 4: surf ring = max_map_points
    case = _case("E.capacity", "E", incs, 0, max_map_points=mm, expect=dict(full_at=(2, 6)))
    case["refused"] = (3, 5)
    return case


# ---- F: many maps in one call ----------------------------------------------------------------------------------------------------

F_CALLS = 10   # calls 0 .. 8 build the contents at different ring ages, call 9 is one more round on top
F_ORDERS = {"F.n1": ["empty"], "F.n2": ["empty", "one"], "F.n3": ["empty", "one", "mixed"],
            "F.n5": ["empty", "one", "mixed", "mixed", "above"],
            "F.n9": ["empty", "one", "mixed", "mixed", "above", "big", "one", "mixed", "empty"],
            "F.n6.empty-last": ["one", "mixed", "mixed", "above", "big", "empty"],
            "F.n6.empty-middle": ["one", "mixed", "mixed", "empty", "above", "big"]}


def _contents(O, above):
    """content name -> {call: (corner, surf)}; calls not named are empty stacks."""
    mc, ms = mixed(257, LEAF[0], 259)[0], mixed(257, LEAF[1], 260)[0]
    big = _split(one_voxel(65537, LEAF[0], 41), B_SIZES[65537])
    small = _split(lattice(300, LEAF[1], 42), [30] * 8 + [60])
    a = above["incs"]
    return {"empty": {},
            "one": {0: (np.array([[0.3, -1.7, 2.2]], F32), EMPTY)},
            "mixed": {3: (mc, ms)},
            "mixed2": {5: (mc, ms)},                       # the SAME cloud in another ring slot: the same concatenation
            "above": {2: (a[0][0], a[0][1]), 6: (a[1][0], a[1][1])},
            "big": {k: (big[k], small[k]) for k in range(9)}}


def cases_F(O, above):
    con = _contents(O, above)
    rng = np.random.default_rng(51)
    extra = [(rng.uniform(-3, 3, (2, 3)).astype(F32), rng.uniform(-3, 3, (1, 3)).astype(F32)) for _ in range(16)]
    out = []
    for name, order in F_ORDERS.items():
        names = []
        for b in order:                                      # the second "mixed" of a run is the twin in the other slot
            names.append("mixed2" if b == "mixed" and names and names[-1] == "mixed" else b)
        calls = []
        for k in range(F_CALLS):
            row = []
            for j, b in enumerate(names):
                c, s = con[b].get(k, (EMPTY, EMPTY))
                if k == F_CALLS - 1 and b != "empty":       # the extra round: every ring but the empty one grows
                    c, s = extra[j]
                row.append((c, s, EYE))
            calls.append(row)
        out.append(dict(name=name, family="F", banks=names, calls=calls, big=names.index("big") if "big" in names else None))
    return out


def bank_case(fcase, j):
    """Bank j of a bank case as a case of its own (for oracle_history and ring_totals)."""
    return dict(name="%s[%d]" % (fcase["name"], j), family="F", incs=[row[j] for row in fcase["calls"]], check_from=0, refused=())


def chunks(pts, budget):
    """The first bank of every chunk of one call: greedy in call order over the banks' ring points after the write; a bank over
    the budget is a chunk of its own."""
    cut, run = [0], 0
    for i, p in enumerate(pts):
        if i > cut[-1] and run + p > budget:
            cut.append(i)
            run = 0
        run += p
    return cut


SINGLE = ["A.i.empty-first", "A.ii.runs", "A.iii.wrap-empties", "A.iv.last-slot"] + ["B.%d" % n for n in B_SIZES] + \
    ["B.257.mixed", "B.65537.mixed", "C.identity", "C.far", "C.negative", "D.below", "D.above"]
KNN = ["B.1", "B.257.mixed", "D.above", "B.65537"]
BANKS = list(F_ORDERS)


def build_cases(O):
    """name -> case, every family."""
    single = cases_A() + cases_B() + cases_C() + cases_D(O)
    by = {c["name"]: c for c in single}
    assert list(by) == SINGLE
    e = case_E()
    by[e["name"]] = e
    for f in cases_F(O, by["D.above"]):
        by[f["name"]] = f
    return by
