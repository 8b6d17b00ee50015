"""GPU suite: the device's own line / plane model fit, reached through the test hook mml_model_fit5 (the __device__ functions
the association and GICP kernels call: eig3_sym, plane_fit5, line_model5, plane_model5), on caller-supplied inputs.
  1. device sqrt and / in double and float are correctly rounded: bit-equal to numpy's on 1e7 arguments each and on the
     near-halfway cases of tests/golden/modelfit_kat.npz;
  2. device == oracle bit for bit (NaN where the oracle has NaN) on every family of the fixture and on 1e7 seeded random
     items per operation;
  3. device against the exact references of the fixture, with the bounds of tests/test_modelfit.py."""
import numpy as np
import pytest

import modelfit_checks as K
from test_modelfit import check_against_exact

pytestmark = pytest.mark.gpu
CHUNK, CHUNKS = 1000000, 10


@pytest.fixture(scope="module")
def ctx(M):
    c = M.Context(max_scans=1, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kat():
    return K.load()


def assert_same_bits(dev, ref, what):
    """bit equality (signed zeros included); a NaN of the oracle must be a NaN on the device"""
    u = np.uint64 if dev.dtype == np.float64 else np.uint32
    nd, nr = np.isnan(dev), np.isnan(ref)
    bad = (nd != nr) | (~nr & (dev.view(u) != ref.view(u)))
    if bad.any():
        rows = np.flatnonzero(bad.reshape(len(dev), -1).any(1))
        i = rows[0]
        raise AssertionError("%s: %d of %d items differ; first item %d\n device %r\n oracle %r" % (what, len(rows), len(dev), i, dev[i], ref[i]))


def random_points(rng, n):
    """(n, 5, 3) float neighbourhoods: edges, planar patches, blobs, lattice points, repeated points; map-like coordinates"""
    kind = rng.integers(0, 8, n)
    c = rng.uniform(-80, 80, (n, 1, 3))
    d = rng.normal(size=(n, 1, 3))
    t = rng.uniform(-1, 1, (n, 5, 1))
    noise = rng.normal(size=(n, 5, 3)) * (10.0 ** rng.uniform(-4, -0.3, (n, 1, 1)))
    p = c + t * d + noise                                                 # an edge with scatter
    e = rng.normal(size=(n, 1, 3))
    patch = c + t * d + rng.uniform(-1, 1, (n, 5, 1)) * e + noise * (kind == 2)[:, None, None]
    p = np.where((kind == 1)[:, None, None] | (kind == 2)[:, None, None], patch, p)
    p = np.where((kind == 3)[:, None, None], c + rng.normal(size=(n, 5, 3)) * 0.3, p)
    p = np.where((kind == 4)[:, None, None], np.round(p / 0.2) * 0.2, p)  # voxel-filter lattice
    flat = p.copy()
    flat[:, :, 2] = c[:, :, 2]
    p = np.where((kind == 5)[:, None, None], flat, p)                     # floor: one exactly constant column
    p = p.astype(np.float32)
    dup = kind == 6                                                       # repeated points, ranks 2 and 1
    p[dup, 4] = p[dup, 3]
    p[dup & (t[:, 0, 0] > 0), 2] = p[dup & (t[:, 0, 0] > 0), 3]
    near = kind == 7                                                      # close to the origin
    p[near] *= np.float32(1e-3)
    return p


def random_items(op, rng, n):
    if op in (K.LINE, K.PLANE, K.QR):
        p = random_points(rng, n)
        if op == K.LINE:
            return p.reshape(n, 15)
        if op == K.PLANE:
            sel = p.mean(1) + rng.normal(size=(n, 3)).astype(np.float32) * np.float32(0.3)
            return np.concatenate([p.reshape(n, 15), sel.astype(np.float32)], 1)
        a = p.reshape(n, 15).astype(np.float64)
        g = rng.random(n) < 0.3                                           # general doubles, all scales
        a[g] = rng.normal(size=(int(g.sum()), 15)) * 10.0 ** rng.uniform(-6, 6, (int(g.sum()), 1))
        return a
    if op == K.EIG3:
        p = random_points(rng, n).astype(np.float64)
        q = p - p.mean(1, keepdims=True)
        S = np.einsum("nji,njk->nik", q, q) / 5
        S = (S.astype(np.float32)).astype(np.float64)                     # float covariances, as the line fit passes them
        S *= 10.0 ** rng.choice([0, 0, 0, -6, 3, -300], (n, 1, 1))
        m = np.stack([S[:, 0, 0], S[:, 1, 0], S[:, 1, 1], S[:, 2, 0], S[:, 2, 1], S[:, 2, 2]], 1)
        k = rng.integers(0, 10, n)
        m[k == 0, 3] = 0.0                                                # m20 = 0: no tridiagonalisation
        m[k == 1, 1] = m[k == 1, 3] = m[k == 1, 4] = 0.0                  # diagonal
        return m
    if op == K.OPS64:
        a = rng.integers(0, 2 ** 63, (n, 2), dtype=np.int64)
        a[:, 1] |= rng.integers(0, 2, n, dtype=np.int64) << 63            # divisors of either sign
        a = a.view(np.float64)
        k = n // 4                                                        # the arguments of the fit: sums of squares of ranges
        r = rng.uniform(0.5, 200, (k, 3))
        a[:k, 0], a[:k, 1] = (r * r).sum(1), r[:, 0] - r[:, 1]
        return a
    a = rng.integers(0, 2 ** 31, (n, 2), dtype=np.int64)
    a[:, 1] |= rng.integers(0, 2, n, dtype=np.int64) << 31
    a = a.astype(np.uint32).view(np.float32)
    k = n // 4
    r = rng.uniform(0.5, 200, (k, 3)).astype(np.float32)
    a[:k, 0], a[:k, 1] = (r * r).sum(1), r[:, 0] - r[:, 1]
    return a


@pytest.mark.parametrize("op", [K.OPS64, K.OPS32], ids=["f64", "f32"])
def test_device_sqrt_and_division_are_correctly_rounded(ctx, kat, op):
    rng = np.random.default_rng(9300 + op)
    sets = [kat["ops64_in" if op == K.OPS64 else "ops32_in"]] + [None] * CHUNKS
    for s in sets:
        a = random_items(op, rng, CHUNK) if s is None else s
        dev = ctx.model_fit5(op, a)
        with np.errstate(all="ignore"):
            ref = np.stack([np.sqrt(a[:, 0]), a[:, 0] / a[:, 1]], 1)
        assert ref.dtype == dev.dtype
        assert_same_bits(dev[:, 0], ref[:, 0], "sqrt")
        assert_same_bits(dev[:, 1], ref[:, 1], "division")


@pytest.mark.parametrize("op,key", [(K.EIG3, "eig3_in"), (K.QR, "qr_in"), (K.LINE, "line_in"), (K.PLANE, "plane_in")],
                         ids=["eig3", "qr", "line", "plane"])
def test_device_fit_equals_oracle_bit_for_bit(ctx, O, kat, op, key):
    assert_same_bits(ctx.model_fit5(op, kat[key]), O.model_fit5(op, kat[key]), "fixture " + key)
    rng = np.random.default_rng(930 + op)
    seen = np.zeros(4)
    for c in range(CHUNKS):
        a = random_items(op, rng, CHUNK)
        dev, ref = ctx.model_fit5(op, a), O.model_fit5(op, a)
        assert_same_bits(dev, ref, "%s chunk %d" % (key, c))
        if op == K.QR:
            seen += np.bincount(ref[:, 3].astype(int), minlength=4)
        elif op != K.EIG3:
            seen[:2] += np.bincount(ref[:, 0].astype(int), minlength=2)
    print(key, "ranks / decisions seen:", seen)
    if op == K.QR:
        assert seen[1] > 0 and seen[2] > 0 and seen[3] > 0      # the random items reach the rank-deficient branches
    elif op != K.EIG3:
        assert seen[0] > CHUNK // 2 and seen[1] > CHUNK // 2    # both sides of the gate, in numbers


def test_device_fit_against_exact(ctx, kat):
    check_against_exact(kat, ctx.model_fit5, "device")


def degenerate_map(rng):
    """A map of isolated clusters of exactly 5 points, 4 m apart (the five at the origin 8 m from the rest), and one feature
    beside each: walls in three orientations and edges, which fix the pose, and the degenerate families of the fixture."""
    shapes = []
    for k in range(12):
        u, v = np.eye(3)[(k + 1) % 3], np.eye(3)[(k + 2) % 3]
        uv = rng.uniform(-0.3, 0.3, (5, 2))
        shapes.append(uv[:, :1] * u + uv[:, 1:] * v)                                 # wall: one exactly constant column
    t = np.array([-0.4, -0.2, 0.0, 0.2, 0.4])[:, None]
    for d in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1]):
        shapes.append(t * np.array(d, float) / np.linalg.norm(d) + rng.normal(size=(5, 3)) * 0.004)   # edges
    shapes.append(t * np.array([1.0, 0, 0]))                                          # exactly collinear
    shapes.append(np.zeros((5, 3)))                                                   # coincident
    shapes.append(np.array([[0, 0, 0]] * 4 + [[0.2, 0, 0]], float))                   # four coincident + one
    shapes.append(rng.integers(-2, 3, (5, 3)) * 0.2)                                  # lattice
    shapes.append(rng.normal(size=(5, 3)) * 0.15)                                     # isotropic blob: neither model
    thick = rng.uniform(-0.3, 0.3, (5, 3))
    thick[:, 2] = [0, 0, 0, 0, 0.45]
    shapes.append(thick)                                                              # a plane with one point far off it
    cen = np.array([[8.0 + 4 * (i % 5), -8.0 + 4 * (i // 5), 2.0 + (i % 3)] for i in range(len(shapes))])
    pts = [c + s for c, s in zip(cen, shapes)] + [np.zeros((5, 3))]                   # ... and five points at (0, 0, 0)
    cen = np.concatenate([cen, np.zeros((1, 3))])
    return np.concatenate(pts).astype(np.float32), cen + np.array([0.05, -0.03, 0.07])


def _arrays(lf, pf):
    return (np.concatenate([lf["point_ori"], lf["p1"], lf["p2"], lf["error"][:, None]], axis=1),
            np.concatenate([pf["point_ori"], pf["point_proj"], pf["omega"], pf["error"][:, None]], axis=1))


@pytest.mark.parametrize("count", [2, 96], ids=["group_search", "fit_all"])
def test_degenerate_clusters_through_associate_and_solve(M, O, count):
    """The degenerate neighbourhoods through the real kernels, in both launch forms (count <= 8: every feature goes to the group
    search; 96 slots: k_associate + k_associate_fit_all), k_assoc_stats and the solve included: records, src, counts,
    min_singular, is_degenerate and the solved pose equal the oracle's, NaN for NaN (convention 13)."""
    from conftest import perturbed, pose_to_x
    world_map, where = degenerate_map(np.random.default_rng(41))
    tree = O.KdTree(world_map)
    T0 = perturbed(np.eye(4))
    feat = ((where - T0[:3, 3]) @ T0[:3, :3]).astype(np.float32)                       # the lidar-frame points that land beside the clusters
    T = np.stack([perturbed(np.eye(4), dt=(0.03 + 2e-4 * s, -0.02, 0.01)) for s in range(count)])
    c = M.Context(max_scans=count, max_velo_points=2048, max_livox_points=2048, device=0)
    try:
        c.map_set_local(0, world_map)
        c.map_set_local(1, world_map)
        for s in range(count):
            c.features_upload(s, 0, feat)
            c.features_upload(s, 1, feat)
        st = c.associate(0, count, T, 1.0)
        x0 = np.stack([pose_to_x(T[s]) for s in range(count)])
        check = sorted({0, count // 2, count - 1})
        ora = {}
        for s in check:
            lf, lsrc = O.associate_lines(feat, tree, T[s], 1.0)
            pf, psrc = O.associate_planes(feat, tree, T[s], 1.0)
            ora[s] = (lf, pf)
            gl, glsrc = c.factors_download(s, 0)
            gp, gpsrc = c.factors_download(s, 1)
            ol, op = _arrays(lf, pf)
            print("slot %d: %d lines, %d planes, %d plane records with a NaN" % (s, len(lf), len(pf), int(np.isnan(op).any(1).sum())))
            assert np.isnan(op[:, 6:9]).any(1).sum() == 1                             # the five points at the origin: accepted, NaN
            assert 0 < len(lf) < len(feat) and 10 < len(pf) < len(feat)               # both gates reject some clusters
            assert np.array_equal(glsrc, lsrc) and np.array_equal(gpsrc, psrc)
            assert np.allclose(gl, ol, rtol=0, atol=1e-9, equal_nan=True) and np.array_equal(np.isnan(gl), np.isnan(ol))
            assert np.allclose(gp, op, rtol=0, atol=1e-9, equal_nan=True) and np.array_equal(np.isnan(gp), np.isnan(op))
            assert st[s].n_line == len(lf) and st[s].n_plane == len(pf)
            with np.errstate(invalid="ignore"):
                assert st[s].n_line_used == int(np.sum(np.abs(lf["error"]) > 1e-5))
                assert st[s].n_plane_used == int(np.sum(np.abs(pf["error"]) > 1e-5))
            ms = O.check_localizability(pf)
            assert (np.isnan(ms) and np.isnan(st[s].min_singular)) or abs(st[s].min_singular - ms) < 1e-9 * max(1.0, abs(ms))
            assert st[s].is_degenerate == int(ms < 3.0)
        xs, summ, _ = c.solve(0, count, x0, np.eye(4), max_iters=10)
        assert np.all(np.isfinite(xs))
        for s in check:
            xo, so, _ = O.solve_window([ora[s][0]], [ora[s][1]], x0[s][None], np.eye(4), 10)
            assert np.all(np.isfinite(xo)) and np.abs(xs[s] - xo[0]).max() < 1e-9
            assert summ[s].iterations == so["iterations"] and summ[s].successful == so["successful"]
    finally:
        c.close()
