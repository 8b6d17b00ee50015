"""Hand-built maps of a few dozen to a few hundred points for the association tests: the builders of the far-query tests
(tests/test_gpu_assoc_far.py) and the cases of the two-level look-up -- the cube cloud of the feature's own cube first, the
local map as fall-back -- that tests/test_assoc_two_level_census.py checks on the oracle alone and
tests/test_gpu_assoc_two_level_forms.py runs on the device.

Geometry of the two-level cases.  c is the grid cell of the kind (5 x leaf).  A "world" is the box [o, o + 20 c]^3 whose
corners and edge midpoints ("anchors") are in every cloud built on it, so a grid over such a cloud has origin o and 21 cells
per axis.  On a face axis o = 25 - 10.5 c: the cube face at 25 m cuts cell 10 in the middle; on the other axes o = -10.5 c.
Positions inside a world are written in cells along a frame (u, v, w): u the face axis, w = u + 2 (mod 3).  A cube is filled up
to a wanted count with lattice points (one a cell) that lie farther than 5.5 c from every feature; every gate used is (5 c)^2
or 25 m^2, so they are never neighbours.  Clouds and features are float32 from the start.

A case is a plain dict:
  name, kind (the kind it is about; None: both), thres (thres_dist), cen, T (4 x 4 pose),
  local = [corner, surf] local maps, glob = [(xyz, cube) or None] * 2 cube clouds with M.cube_index of every point,
  feats = [corner, surf] features,
  expect = [per kind: dict(n = factors, n_cube = factors of the cube stage, none = features without a factor)],
  far = whether a 12-slot call has far queries, cells = what the builder asserted about grid cells (for the reader)."""
import numpy as np

F32 = np.float32
GATE = (100, 50)          # a cube is used when it holds MORE corner / surf points (Estimator.cpp:198, :627)
CUBE_DIM = (21, 21, 11)   # cubes along x, y, z
CEN_AXIS = (2, 0, 1)      # the entry of cen that belongs to x, y, z


def _cells(ctx):
    """The grid cells of the two kinds as the library derives them: the configured cell, else 5 x leaf in float.  ctx: a
    context or its configuration."""
    cfg = getattr(ctx, "cfg", ctx)
    f = np.float32
    return (float(f(cfg.cell_corner) if cfg.cell_corner > 0 else f(5.0) * f(cfg.leaf_corner)),
            float(f(cfg.cell_surf) if cfg.cell_surf > 0 else f(5.0) * f(cfg.leaf_surf)))


def _anchors(c, queries, keep_off, dims=(20, 20, 20)):
    """Corners and edge midpoints of the box [0, dims * c], without those nearer than keep_off to a query."""
    g = [np.array([0.0, d / 2.0, float(d)]) * c for d in dims]
    pts = np.array([[x, y, z] for i, x in enumerate(g[0]) for j, y in enumerate(g[1]) for k, z in enumerate(g[2])
                    if (i == 1) + (j == 1) + (k == 1) <= 1])
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    far = np.all(np.linalg.norm(pts[:, None, :] - q[None], axis=2) > keep_off, axis=1)
    pts = pts[far]
    assert np.all(pts.min(0) == 0) and np.all(pts.max(0) == np.array(dims) * c) and len(pts) >= 17
    return pts


def _five(kind, base, step, a, b=None):
    """Five points at `base` and beyond along unit axis vectors: a line along a (corner kind), a quincunx in the a / b plane
    (surf kind).  base + multiples of step: the other four are base + step * (...)."""
    base, a = np.asarray(base, np.float64), np.asarray(a, np.float64)
    if kind == 0:
        return np.array([base + j * step * a for j in range(5)])
    b = np.asarray(b, np.float64)
    return np.array([base, base + step * (a + b), base + step * (a - b), base + 2 * step * (a + b), base + 2 * step * (a - b)])


def _dummy(c):
    """A map and one feature for the kind a case does not look at."""
    q = np.array([[10.5 * c, 10.5 * c, 10.5 * c]])
    faces = np.array([[10, 10, 0], [10, 10, 20], [10, 0, 10], [10, 20, 10], [0, 10, 10], [20, 10, 10]]) * c
    return np.concatenate([_anchors(c, q, 0.0), faces]), q


def _centre(c):
    return np.array([10.5, 10.5, 10.5]) * c


# ---------------------------------------------------------------------------------------------------------------------------
# the two-level cases

def _frame(ax):
    e = np.eye(3)
    return e[ax], e[(ax + 1) % 3], e[(ax + 2) % 3]


def _origin(c, faces):
    o = np.full(3, -10.5 * c)
    o[list(faces)] = 25.0 - 10.5 * c
    return o


def _at(p, fr, c, u, v, w):
    return np.asarray(p, np.float64) + c * (u * fr[0] + v * fr[1] + w * fr[2])


def _clean(kind, p, fr, c, u, v, w, lift=0.0):
    """A clean model from (u, v, w) cells off p: a line along v / a quincunx in the v-w plane, within 0.2 c; `lift` metres off
    across the model (along w for the line, along u for the plane)."""
    base = _at(p, fr, c, u, v, w) + lift * (fr[2] if kind == 0 else fr[0])
    return _five(kind, base, 0.05 * c, fr[1], fr[2])


def _broken(kind, p, fr, c, u, v, w, away, lift=0.0):
    """Five points that pass the distance gate and yield no model: corner kind an isotropic blob of radius 0.2 c (variances
    0.016, 0.016, 0.0064 c^2: ev[2] <= 3 ev[1]); surf kind a 0.8 c square across u and a fifth point 0.8 c off its centre along
    `away` * u: the fitted plane stays across u, about 0.16 c off the square, and ends 0.64 c = 0.64 m from the fifth point (a
    small square would not do: a plane through its centre and the fifth point passes within 0.2 m of all five)."""
    g = _at(p, fr, c, u, v, w) + lift * (fr[2] if kind == 0 else fr[0])
    if kind == 0:
        return np.array([g + 0.2 * c * d for d in (fr[0], -fr[0], fr[1], -fr[1], fr[2])])
    sq = [g + 0.4 * c * (a * fr[1] + b * fr[2]) for a in (-1, 1) for b in (-1, 1)]
    return np.array(sq + [g + away * 0.8 * c * fr[0]])


def cell_of(p, origin, c):
    """Grid cell of points in a grid of origin `origin` and cell c, in the library's arithmetic (cell_coord, unclamped)."""
    p = np.asarray(p, F32).reshape(-1, 3)
    return np.floor((p - np.asarray(origin, F32)) * (F32(1.0) / F32(c))).astype(int)


def _lattice(c, lo, n=(20, 20, 20)):
    ax = [lo[k] + (np.arange(n[k]) + 0.5) * c for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


def _fill(M, cen, pts, lattice, feats, c, targets):
    """pts and lattice points until cube `id` holds targets[id] points; the lattice points used lie > 5.5 c from every feature."""
    pts = np.asarray(pts, F32)
    lat = np.asarray(lattice, F32)
    f = np.asarray(feats, np.float64).reshape(-1, 3)
    f = f[np.all(np.isfinite(f), axis=1)]
    lat = lat[np.all(np.linalg.norm(lat[:, None, :].astype(np.float64) - f[None], axis=2) > 5.5 * c, axis=1)]
    lcube = M.cube_index(lat, cen)
    have = M.cube_index(pts, cen)
    out = [pts]
    for cid, want in targets.items():
        need = want - int(np.sum(have == cid))
        cand = lat[lcube == cid]
        assert 0 <= need <= len(cand), (cid, want, need, len(cand))
        out.append(cand[:need])
    pts = np.concatenate(out)
    cube = M.cube_index(pts, cen)
    assert np.all(cube < 4851)
    for cid, want in targets.items():
        assert int(np.sum(cube == cid)) == want
    return pts, cube


def _sparse(pts, c):
    """At most 12 points per occupied cell on average: the grid build keeps the configured cell (grid_cell_rule.h)."""
    cells = np.unique(cell_of(pts, np.asarray(pts, F32).min(0), c), axis=0)
    return len(pts) <= 12 * len(cells)


def _knn(pts, q, k=5):
    """Indices of the k nearest of pts to q by float d2, ties by index."""
    d = ((np.asarray(pts, F32) - np.asarray(q, F32)) ** 2).sum(1, dtype=F32)
    return np.lexsort((np.arange(len(d)), d))[:k]


def _box_anchors(c, o, feats, drop_cube=None, M=None, cen=None):
    a = _anchors(c, np.asarray(feats, np.float64).reshape(-1, 3) - o, 5.5 * c) + o
    if drop_cube is not None:
        a = a[M.cube_index(a, cen) != drop_cube]
        assert np.all(a.min(0) == o) and np.all(a.max(0) == o + 20 * c)
    return a


def _case(M, name, kind, c_all, cen, thres, feats, local, glob, expect, far=False, T=None, cells=None):
    """Puts the kind under test beside an idle other kind (_dummy: one feature, no neighbour within any gate used)."""
    dm, df = _dummy(c_all[1 - kind])
    case = dict(name=name, kind=kind, thres=float(thres), cen=tuple(cen), T=np.eye(4) if T is None else T, far=far, cells=cells,
                local=[None, None], glob=[None, None], feats=[None, None], expect=[None, None])
    case["local"][kind] = np.ascontiguousarray(local, F32)
    case["local"][1 - kind] = np.ascontiguousarray(dm, F32)
    case["glob"][kind] = None if glob is None else (np.ascontiguousarray(glob[0], F32), np.ascontiguousarray(glob[1], np.int32))
    case["feats"][kind] = np.ascontiguousarray(feats, F32).reshape(-1, 3)
    case["feats"][1 - kind] = np.ascontiguousarray(df, F32)
    case["expect"][kind] = expect
    case["expect"][1 - kind] = dict(n=0, n_cube=0, none=[0])
    for m in case["local"]:
        assert _sparse(m, c_all[kind]) or len(m) < 64
    if glob is not None:
        assert _sparse(glob[0], c_all[kind])
    return case


def _expect(n_feat, cube=(), local=()):
    got = sorted(list(cube) + list(local))
    return dict(n=len(got), n_cube=len(cube), none=[i for i in range(n_feat) if i not in got])


DEFAULT_CEN = (10, 5, 10)


def _face_world(M, kind, c, faces, side, du):
    """World with the given face axes; the feature `du` metres (du < 1) or cells off the face on side `side` of every face."""
    o = _origin(c, faces)
    fr = _frame(faces[0])
    g0 = o + 10.5 * c          # the box centre: on every face axis the face itself
    F = g0.copy()
    for ax in faces:
        F[ax] += side * du
    F = F.astype(F32).astype(np.float64)
    return o, fr, g0, F


def case_count_gate(M, cfg, kind, count, n_local=None, with_cube=True):
    """A: the cube of the feature holds exactly `count` points of the kind, five of them a clean model beside the feature; the
    local map is the same model lifted by 5 cm (and anchors: 25 points, or exactly n_local)."""
    cs = _cells(cfg)
    c = cs[kind]
    o, fr, g0, F = _face_world(M, kind, c, (0,), -1, 0.01)
    own = int(M.cube_index(F[None], DEFAULT_CEN)[0])
    anchors = _box_anchors(c, o, F)
    near = _clean(kind, g0, fr, c, -0.3, -0.1, 0.05)
    glob = None
    if with_cube:
        glob = _fill(M, DEFAULT_CEN, np.concatenate([near, anchors]), _lattice(c, o), F, c, {own: count})
        assert np.array_equal(np.sort(_knn(glob[0][glob[1] == own], F)), np.arange(5))
    lifted = _clean(kind, g0, fr, c, -0.3, -0.1, 0.05, lift=0.05)
    local = np.concatenate([lifted, anchors if n_local is None else anchors[:n_local - 5]])
    assert n_local is None or len(local) == n_local
    in_cube = with_cube and count > GATE[kind]
    in_local = not in_cube and len(local) > 20
    name = "A-%s-cube%s-local%d" % ("cs"[kind], count if with_cube else "none", len(local))
    return _case(M, name, kind, cs, DEFAULT_CEN, (5 * c) ** 2, F[None], local, glob,
                 _expect(1, cube=[0] if in_cube else [], local=[0] if in_local else []))


def case_tags_near(M, cfg, kind, where):
    """B: the feature 1 cm inside its cube at a face; five points of the neighbouring cube(s) are nearer than any of its own and
    lie in the feature's home cell; its own five lie in the home cell ("y") or in ring 1 ("x", "mirror", "corner")."""
    cs = _cells(cfg)
    c = cs[kind]
    faces = {"x": (0,), "mirror": (0,), "y": (1,), "corner": (0, 1)}[where]
    side = 1 if where == "mirror" else -1
    o, fr, g0, F = _face_world(M, kind, c, faces, side, 0.01)
    own = int(M.cube_index(F[None], DEFAULT_CEN)[0])
    if where == "corner":
        # cubes: own (x < 25, y < 25), beyond x (v < 0 keeps y < 25), beyond y (u < 0 keeps x < 25); the fourth stays empty
        other = np.concatenate([_clean(kind, g0, fr, c, 0.06, -0.3, 0.03), _clean(kind, g0, fr, c, -0.1, 0.06, 0.03)])
        mine = (-0.8, -0.45, 0.03)
        empty = int(M.cube_index((g0 + 1.0)[None], DEFAULT_CEN)[0])
    else:
        other = _clean(kind, g0, fr, c, -side * 0.06, -0.1, 0.03)
        mine = (side * (0.35 if where == "y" else 0.8), -0.1, 0.03)
        empty = None
    five = _clean(kind, g0, fr, c, *mine)
    anchors = _box_anchors(c, o, F, empty, M, DEFAULT_CEN)
    pts, cube = _fill(M, DEFAULT_CEN, np.concatenate([five, other, anchors]), _lattice(c, o), F, c, {own: GATE[kind] + 1})
    assert np.all(cube[:5] == own) and np.all(cube[5:5 + len(other)] != own) and (empty is None or not np.any(cube == empty))
    assert np.all(cube[_knn(pts, F)] != own), "the five nearest points belong to other cubes"
    assert np.array_equal(np.sort(np.flatnonzero(cube == own)[_knn(pts[cube == own], F)]), np.arange(5))
    home = cell_of(F, o, c)[0]
    assert np.all(cell_of(other, o, c) == home), "the other cubes' points share the feature's home cell"
    ring = np.abs(cell_of(five, o, c) - home).max(1)
    assert np.all(ring == (0 if where == "y" else 1))
    local = np.concatenate([_clean(kind, g0, fr, c, *mine, lift=0.05), anchors])
    return _case(M, "B-%s-%s" % ("cs"[kind], where), kind, cs, DEFAULT_CEN, (5 * c) ** 2, F[None], local, (pts, cube),
                 _expect(1, cube=[0]), cells=dict(home=home.tolist(), own_ring=ring.tolist()))


def case_tags_far(M, cfg, kind, dist):
    """C: as B at the x face, the own-cube model `dist` cells away (3, 4: inside the gate of 5 c; 5.2: beyond it) with two more
    own-cube points of the same line / plane in ring 1: ring 1 ends with two tagged entries, the feature is queued with them."""
    cs = _cells(cfg)
    c = cs[kind]
    o, fr, g0, F = _face_world(M, kind, c, (0,), -1, 0.01)
    own = int(M.cube_index(F[None], DEFAULT_CEN)[0])
    other = _clean(kind, g0, fr, c, 0.06, -0.1, 0.03)
    extras = np.array([_at(g0, fr, c, -0.35, 0.6, 0.03), _at(g0, fr, c, -0.35, 0.9, 0.03)])
    five = _clean(kind, g0, fr, c, -0.35, dist + 0.1, 0.03)
    anchors = _box_anchors(c, o, F)
    pts, cube = _fill(M, DEFAULT_CEN, np.concatenate([extras, five, other, anchors]), _lattice(c, o), F, c, {own: GATE[kind] + 1})
    home = cell_of(F, o, c)[0]
    ring = np.abs(cell_of(pts[cube == own], o, c) - home).max(1)
    assert int(np.sum(ring <= 1)) == 2 and np.all(np.abs(cell_of(extras, o, c) - home).max(1) == 1)
    far_ring = np.abs(cell_of(five, o, c) - home).max(1)
    inside = dist < 5
    assert np.all(far_ring == dist) if inside else np.all(far_ring >= 5), far_ring
    d = np.linalg.norm(five - F, axis=1)
    assert np.all(d < 4.99 * c) if inside else np.all(d > 5.01 * c)
    assert np.all(cube[_knn(pts, F)] != own)
    if inside:
        local = np.concatenate([extras + 0.05 * (fr[2] if kind == 0 else fr[0]), _clean(kind, g0, fr, c, -0.35, dist + 0.1, 0.03, lift=0.05), anchors])
        exp = _expect(1, cube=[0])
    else:
        local = np.concatenate([_clean(kind, g0, fr, c, -0.35, -0.1, 0.03, lift=0.05), anchors])
        exp = _expect(1, local=[0])
    return _case(M, "C-%s-%s" % ("cs"[kind], dist), kind, cs, DEFAULT_CEN, (5 * c) ** 2, F[None], local, (pts, cube), exp, far=True,
                 cells=dict(home=home.tolist(), own_ring=far_ring.tolist()))


def case_fall_back(M, cfg, kind, variant):
    """D (i) .. (v): the own-cube neighbourhood passes the gate and yields no model (v: four inside the gate, the fifth beyond);
    the local map holds a clean model in rings 0-1 (i, v), three cells out (ii), no model (iii), or 20 points (iv)."""
    cs = _cells(cfg)
    c = cs[kind]
    o, fr, g0, F = _face_world(M, kind, c, (0,), -1, 0.25 * c)
    own = int(M.cube_index(F[None], DEFAULT_CEN)[0])
    anchors = _box_anchors(c, o, F)
    if variant == "v":
        mine = np.concatenate([_clean(kind, F, fr, c, -0.1, -0.1, 0.03)[:4], _at(F, fr, c, -0.1, 5.2, 0.03)[None]])
    else:
        mine = _broken(kind, F, fr, c, -0.1, 0.0, 0.0, -1)
    pts, cube = _fill(M, DEFAULT_CEN, np.concatenate([mine, anchors]), _lattice(c, o), F, c, {own: GATE[kind] + 1})
    assert np.all(cube[:5] == own)
    nn = np.flatnonzero(cube == own)[_knn(pts[cube == own], F)]
    assert np.array_equal(np.sort(nn), np.arange(5))
    d5 = np.linalg.norm(pts[nn[4]].astype(np.float64) - F)
    assert d5 > 5.01 * c if variant == "v" else d5 < c
    near = _clean(kind, F, fr, c, -0.15, -0.1, 0.05, lift=0.05)
    if variant in ("i", "v"):
        local, ok = np.concatenate([near, anchors]), True
    elif variant == "ii":
        out = _clean(kind, F, fr, c, -0.15, 3.1, 0.05)
        assert np.all(np.abs(cell_of(out, o, c) - cell_of(F, o, c)[0]).max(1) == 3)
        local, ok = np.concatenate([out, anchors]), True
    elif variant == "iii":
        local, ok = np.concatenate([_broken(kind, F, fr, c, -0.1, 0.0, 0.0, -1, lift=0.05), anchors]), False
    else:
        local, ok = np.concatenate([near, anchors[:15]]), False
        assert len(local) == 20
    return _case(M, "D-%s-%s" % ("cs"[kind], variant), kind, cs, DEFAULT_CEN, (5 * c) ** 2, F[None], local, (pts, cube),
                 _expect(1, local=[0] if ok else []), far=variant in ("ii", "v"))


SITES = ((4.5, 4.5), (4.5, 15.5), (15.5, 4.5), (15.5, 15.5))   # (v, w) cells of the four features of D (vi)


def _mixed_world(M, kind, c):
    """D (vi): four features 11 cells apart in one cube, 0.25 c inside the x face.
      0: a clean own-cube model beside it: finishes in the cube;
      1: nothing of its cube in rings 0-1, five without a model three cells out: queued far in the cube stage, the fit fails (the
         mark of k_associate_fit), the local map has a clean model beside it;
      2: five without a model beside it: parked ready, the fit fails (the append of k_associate_fit_all), local model beside it;
      3: nothing of its cube in rings 0-1, a clean own-cube model three cells out: an ordinary far entry that ends in the cube."""
    o = _origin(c, (0,))
    fr = _frame(0)
    Fs = []
    for v, w in SITES:
        p = o + np.array([10.5, v, w]) * c
        p[0] -= 0.25 * c
        Fs.append(p)
    Fs = np.array(Fs).astype(F32).astype(np.float64)
    fd = [1.0 if v < 10 else -1.0 for v, w in SITES]
    own = int(M.cube_index(Fs[:1], DEFAULT_CEN)[0])
    assert np.all(M.cube_index(Fs, DEFAULT_CEN) == own)
    anchors = _box_anchors(c, o, Fs)
    mine = [_clean(kind, Fs[0], fr, c, -0.1, -0.1, 0.03),
            _broken(kind, Fs[1], fr, c, -0.1, fd[1] * 3.0, 0.0, -1),
            _broken(kind, Fs[2], fr, c, -0.1, 0.0, 0.0, -1),
            _clean(kind, Fs[3], fr, c, -0.1, fd[3] * 3.1, 0.03)]
    pts, cube = _fill(M, DEFAULT_CEN, np.concatenate(mine + [anchors]), _lattice(c, o), Fs, c, {own: GATE[kind] + 40})
    for s in range(4):
        nn = _knn(pts, Fs[s])
        assert np.array_equal(np.sort(nn), np.arange(5 * s, 5 * s + 5)), (s, nn)
        ring = np.abs(cell_of(pts[nn], o, c) - cell_of(Fs[s], o, c)[0]).max(1)
        assert np.all(ring == 3) if s in (1, 3) else np.all(ring <= 1), (s, ring)
    local = np.concatenate([_clean(kind, Fs[0], fr, c, -0.1, -0.1, 0.03, lift=0.05),
                            _clean(kind, Fs[1], fr, c, -0.15, -0.1, 0.05, lift=0.05),
                            _clean(kind, Fs[2], fr, c, -0.15, -0.1, 0.05, lift=0.05),
                            _clean(kind, Fs[3], fr, c, -0.1, fd[3] * 3.1, 0.03, lift=0.05), anchors])
    return Fs, local, (pts, cube)


def case_mixed(M, cfg, kind):
    cs = _cells(cfg)
    c = cs[kind]
    Fs, local, glob = _mixed_world(M, kind, c)
    return _case(M, "D-%s-vi" % "cs"[kind], kind, cs, DEFAULT_CEN, (5 * c) ** 2, Fs, local, glob,
                 _expect(4, cube=[0, 3], local=[1, 2]), far=True)


def edge_points(ax, cen):
    """E: the positions on axis `ax` where the cube index changes or ends, as (coordinate, inside the grid) pairs: 25 and -25 and
    the floats below them; the top face of the cube grid (the float below it is the last inside) and the bottom face (the reference
    decrements at a negative x + 25 even when the quotient is whole: the face itself is outside, the float above it inside)."""
    hi = F32(50.0 * (CUBE_DIM[ax] - cen[CEN_AXIS[ax]]) - 25.0)
    lo = F32(-50.0 * cen[CEN_AXIS[ax]] - 25.0)
    dn, up = F32(-np.inf), F32(np.inf)
    return [(F32(25.0), True), (np.nextafter(F32(25.0), dn), True), (F32(-25.0), True), (np.nextafter(F32(-25.0), dn), True),
            (np.nextafter(hi, dn), True), (hi, False), (np.nextafter(lo, up), True), (lo, False)]


def case_cube_edges(M, cfg, kind, ax, cen):
    """E: eight features on axis `ax` (edge_points), 3 c and -2 c on the other two.  On either side of each of the four faces
    a clean model of the cube on that side (0.2 c below, 0.3 c above; none beyond the grid), every such cube filled above its
    gate; the local map holds all eight models lifted by 5 cm."""
    cs = _cells(cfg)
    c = cs[kind]
    fr = _frame(ax)
    edges = edge_points(ax, cen)
    feats = np.array([float(x) * fr[0] + 3.0 * c * fr[1] - 2.0 * c * fr[2] for x, _ in edges])
    models, lifted, targets, lat = [], [], {}, []
    for j in (0, 2, 4, 6):
        face = float(max(edges[j][0], edges[j + 1][0]))
        p = face * fr[0] + 3.0 * c * fr[1] - 2.0 * c * fr[2]
        lat.append(_lattice(c, p - 10.0 * c))
        for u in (-0.2, 0.3):
            m = _clean(kind, p, fr, c, u, -0.1, 0.03)   # (the model spans v and w only: it stays on its side of the face)
            lifted.append(_clean(kind, p, fr, c, u, -0.1, 0.03, lift=0.05 if u > 0 or kind == 0 else -0.05))
            cid = M.cube_index(m, cen)
            assert np.all(cid == cid[0])
            if cid[0] != 5000:
                models.append(m)
                targets[int(cid[0])] = GATE[kind] + 1
    assert len(targets) == 5 and len(models) == 6   # (the cube between -25 and 25 holds two of the models)
    pts, cube = _fill(M, cen, np.concatenate(models), np.concatenate(lat), feats, c, targets)
    local = np.concatenate(lifted + [np.concatenate(lat)[:20]])
    inside = [i for i, (_, ok) in enumerate(edges) if ok]
    return _case(M, "E-%s-%s-cen%d" % ("cs"[kind], "xyz"[ax], cen[0]), kind, cs, cen, (5 * c) ** 2, feats, local, (pts, cube),
                 _expect(8, cube=inside))


def case_nan(M, cfg, kind, what):
    """E: count-gate case A above the gate with a NaN in a coordinate of features 1 .. 3 ("feature": feature 0 keeps its factor)
    or in the pose's translation ("pose": no factor at all)."""
    case = case_count_gate(M, cfg, kind, GATE[kind] + 1)
    case["name"] = "E-%s-nan-%s" % ("cs"[kind], what)
    if what == "feature":
        f = np.repeat(case["feats"][kind], 4, axis=0)
        for i in range(3):
            f[1 + i, i] = np.nan
        case["feats"][kind] = f
        case["expect"][kind] = _expect(4, cube=[0])
    else:
        case["T"] = np.eye(4)
        case["T"][1, 3] = np.nan
        case["expect"][kind] = _expect(1)
    return case


def case_both_kinds(M, cfg, n_pool=257):
    """F: the maps of D (vi) for both kinds in one case, gate 25 m^2, and a pool of n_pool features per kind: the four features of
    D (vi) in turn, moved by up to 0.02 c.  What each gets is the oracle's business; a prefix of the pool is a valid feature set."""
    cs = _cells(cfg)
    rng = np.random.default_rng(7)
    case = dict(name="F-both", kind=None, thres=25.0, cen=DEFAULT_CEN, T=np.eye(4), far=True, cells=None,
                local=[], glob=[], feats=[], expect=[None, None])
    for kind in (0, 1):
        c = cs[kind]
        Fs, local, glob = _mixed_world(M, kind, c)
        pool = Fs[np.arange(n_pool) % 4] + rng.uniform(-0.02 * c, 0.02 * c, (n_pool, 3))
        assert _sparse(local, c) and _sparse(glob[0], c)
        case["local"].append(np.ascontiguousarray(local, F32))
        case["glob"].append((np.ascontiguousarray(glob[0], F32), np.ascontiguousarray(glob[1], np.int32)))
        case["feats"].append(np.ascontiguousarray(pool, F32))
    return case


def all_cases(M, cfg):
    """Every case of A .. E, by name."""
    out = []
    for kind in (0, 1):
        g = GATE[kind]
        out += [case_count_gate(M, cfg, kind, g), case_count_gate(M, cfg, kind, g + 1)]
        for n_local in (20, 21):
            out += [case_count_gate(M, cfg, kind, g, n_local, with_cube=False), case_count_gate(M, cfg, kind, g, n_local)]
        out += [case_tags_near(M, cfg, kind, w) for w in ("x", "y", "mirror", "corner")]
        out += [case_tags_far(M, cfg, kind, d) for d in (3, 4, 5.2)]
        out += [case_fall_back(M, cfg, kind, v) for v in ("i", "ii", "iii", "iv", "v")]
        out.append(case_mixed(M, cfg, kind))
        out += [case_cube_edges(M, cfg, kind, ax, cen) for ax in (0, 1, 2) for cen in ((10, 5, 10), (3, 3, 3))]
        out += [case_nan(M, cfg, kind, w) for w in ("feature", "pose")]
    return {c["name"]: c for c in out}


def case_names():
    """The names of all_cases, in its order, without building anything (for a parametrised test)."""
    names = []
    for kind in (0, 1):
        k, g = "cs"[kind], GATE[kind]
        names += ["A-%s-cube%d-local25" % (k, g), "A-%s-cube%d-local25" % (k, g + 1)]
        for n_local in (20, 21):
            names += ["A-%s-cubenone-local%d" % (k, n_local), "A-%s-cube%d-local%d" % (k, g, n_local)]
        names += ["B-%s-%s" % (k, w) for w in ("x", "y", "mirror", "corner")]
        names += ["C-%s-%s" % (k, d) for d in (3, 4, 5.2)]
        names += ["D-%s-%s" % (k, v) for v in ("i", "ii", "iii", "iv", "v", "vi")]
        names += ["E-%s-%s-cen%d" % (k, a, cen) for a in "xyz" for cen in (10, 3)]
        names += ["E-%s-nan-%s" % (k, w) for w in ("feature", "pose")]
    return names


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle's answer for a case

def factor_arrays(lf, pf):
    ol = np.concatenate([lf["point_ori"], lf["p1"], lf["p2"], lf["error"][:, None]], axis=1)
    op = np.concatenate([pf["point_ori"], pf["point_proj"], pf["omega"], pf["error"][:, None]], axis=1)
    return ol, op


def oracle_maps(O, case, local=None, cube=True):
    """(cube maps, kd-trees) of the case for the oracle; `local`: other local maps; cube=False: the cube clouds left out (an empty
    cube map that still carries the case's cen)."""
    none = (np.zeros((0, 3), F32), np.zeros(0, np.int32))
    gm = [O.CubeMap(*((case["glob"][k] if cube and case["glob"][k] is not None else none) + (case["cen"],))) for k in (0, 1)]
    tr = [O.KdTree((local or case["local"])[k]) for k in (0, 1)]
    return gm, tr


def oracle_answer(O, case, feats=None, local=None, cube=True):
    """[(records n x 10, src, from_global)] for the two kinds."""
    gm, tr = oracle_maps(O, case, local, cube)
    feats = feats or case["feats"]
    lf, lsrc, lfg = O.associate_lines2(feats[0], gm[0], tr[0], case["T"], case["thres"])
    pf, psrc, pfg = O.associate_planes2(feats[1], gm[1], tr[1], case["T"], case["thres"])
    ol, op = factor_arrays(lf, pf)
    return [(ol, lsrc, lfg), (op, psrc, pfg)]
