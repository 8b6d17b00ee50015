"""Known answers for the line / plane model fit (eig3_sym, plane_fit5, the float tail around them), computed without either
implementation: the inputs are floats or doubles, so every quantity below is a rational number (fractions.Fraction) or an
eigen-system of a rational matrix taken at 50 digits (mpmath), rounded once.  Data only: tests/golden/modelfit_kat.npz.

    python tests/golden/make_modelfit_kat.py [seed]

Families are named in *_families; *_fam holds the family index of every item.  The decision margins stored here and the
*_band constants say which items sit too close to a threshold to be decided against the exact answer; the generator asserts
that outside the threshold families at most 0.1 % of a family are that close, using the exact values alone.
"""
import os
import sys
from fractions import Fraction as Fr

import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = 2.0 ** -52
EPSF = 2.0 ** -23
# Bands inside which a decision is left to the oracle alone (tests/test_modelfit.py checks that its value bounds fit in them):
# line gate  |ev2 - 3 ev1| <= LINE_BAND * (EPSF * (max|A| + max|p| sqrt(max|A|)) + (EPSF max|p|)^2)   (centroid and covariance are accumulated in float)
# 0.2 gate   ||r| - 0.2|   <= (PLANE_BAND * EPSF + QR_BAND * EPS * kappa^2) * (max|p| + 1)
# rank       the pivot's squared norm within a factor RANK_BAND of Eigen's threshold
LINE_BAND, PLANE_BAND, QR_BAND, RANK_BAND = 64.0, 64.0, 256.0, 4.0


def f32(a):
    return np.asarray(a, np.float32)


def ulps32(v, k):
    return (f32(v).view(np.int32) + np.int32(k)).view(np.float32)


def ulps64(v, k):
    return (np.asarray(v, np.float64).view(np.int64) + np.int64(k)).view(np.float64)


def fr(x):
    return Fr(float(x))


def rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


# ---------------------------------------------------------------------------------------------------------------------------
# eig3
def eig_exact(m6):
    """eigenvalues ascending (50 digits) of the symmetric matrix given by its lower triangle m00 m10 m11 m20 m21 m22"""
    a = [mp.mpf(float(v)) for v in m6]
    A = mp.matrix([[a[0], a[1], a[3]], [a[1], a[2], a[4]], [a[3], a[4], a[5]]])
    if all(v == 0 for v in a):
        return [mp.mpf(0)] * 3, None
    s = max(abs(v) for v in a)
    E = mp.eigsy(A / s, eigvals_only=True)
    order = sorted(range(3), key=lambda i: E[i])
    return [E[i] * s for i in order], None


def low6(S):
    return [S[0, 0], S[1, 0], S[1, 1], S[2, 0], S[2, 1], S[2, 2]]


def eig3_families(rng):
    fam = {}
    it = []
    for _ in range(400):
        R = rot(rng)
        d = np.sort(rng.uniform(0, 1, 3)) * 10.0 ** rng.uniform(-8, 2)
        it.append(low6(R @ np.diag(d) @ R.T))
    fam["psd_scales"] = it
    fam["diagonal"] = [[d[0], 0, d[1], 0, 0, d[2]] for d in rng.uniform(0, 1, (150, 3)) * 10.0 ** rng.uniform(-6, 1, (150, 1))]
    it = []
    for _ in range(200):
        m = low6((lambda B: B @ B.T)(rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, 0)))
        m[3] = 0.0 if rng.random() < 0.7 else 10.0 ** rng.uniform(-170, -150)  # m20^2 <= tol either way
        it.append(m)
    fam["m20_zero"] = it
    it = []
    for _ in range(200):
        u = rng.normal(size=3) * 10.0 ** rng.uniform(-3, 1)
        it.append(low6(np.outer(u, u)))
    fam["rank1"] = it
    it = []
    for _ in range(200):
        R = rot(rng)
        a, b = rng.uniform(0.01, 1, 2)
        d = [a, a, b] if rng.random() < 0.5 else [a, b, b]
        it.append(low6(R @ np.diag(d) @ R.T))
    for a in rng.uniform(1e-4, 1, 50):  # exactly repeated
        it.append([a, 0, a, 0, 0, a * 2])
        it.append([a, 0, a * 4, 0, 0, a])
    fam["two_equal"] = it
    fam["three_equal"] = [[a, 0, a, 0, 0, a] for a in 10.0 ** rng.uniform(-8, 2, 60)] + \
                         [low6(a * (rot(rng) @ rot(rng).T)) for a in rng.uniform(0.01, 1, 60)]
    fam["zero"] = [[0.0] * 6, [0.0, 0, 0, 0, 0, -0.0], [-0.0] * 6]
    it = []
    for _ in range(300):  # off-diagonals within a factor 4 of the deflation test |e| <= (|d_i| + |d_i+1|) * 2 eps
        d = rng.uniform(0.1, 1, 3)
        d /= d.max()
        f1, f2 = 4.0 ** rng.uniform(-1, 1, 2)
        e0 = (d[0] + d[1]) * 2 * EPS * f1 * rng.choice([-1, 1])
        e1 = (d[1] + d[2]) * 2 * EPS * f2 * rng.choice([-1, 1])
        m20 = 0.0 if rng.random() < 0.5 else (d[0] + d[2]) * 2 * EPS * rng.uniform(0.25, 4)
        it.append([d[0], e0, d[1], m20, e1, d[2]])
    fam["deflation_edge"] = it
    it = []
    for _ in range(150):
        B = rng.normal(size=(3, 3))
        it.append(low6(B @ B.T * 10.0 ** rng.uniform(-320, -305)))
    fam["denormal"] = it
    it = []
    for _ in range(60):  # float covariances whose ev2 / ev1 is within a few float ulps of 3 (diagonal: the gate is exact there)
        f = f32(rng.uniform(1e-3, 1e-1))
        for k in range(-3, 4):
            big = float(ulps32(f32(3.0) * f, k))
            p = rng.permutation([float(f) * rng.uniform(0, 0.9), float(f), big])
            it.append([p[0], 0, p[1], 0, 0, p[2]])
    fam["gate3"] = it
    return fam


# ---------------------------------------------------------------------------------------------------------------------------
# qr / plane
def solve3(G, b):
    """Gaussian elimination over the rationals"""
    n = len(b)
    M = [list(G[i]) + [b[i]] for i in range(n)]
    for c in range(n):
        p = next((r for r in range(c, n) if M[r][c] != 0), None)
        if p is None:
            return None
        M[c], M[p] = M[p], M[c]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c] / M[c][c]
                M[r] = [x - f * y for x, y in zip(M[r], M[c])]
    return [M[i][n] / M[i][i] for i in range(n)]


def qr_exact(A):
    """A: 5 x 3 floats/doubles.  Exact column-pivoted elimination: the pivot order Eigen would take on exact quantities
    (largest remaining column norm, first maximum), the rank by Eigen's threshold, the basic least-squares solution of
    A X = -1 on the leading block, its residual norm, kappa(A), and the rank margin."""
    A = [[fr(v) for v in row] for row in A]
    cols = [[A[r][c] for r in range(5)] for c in range(3)]
    dot = lambda u, v: sum(x * y for x, y in zip(u, v))
    n2 = [dot(c, c) for c in cols]
    maxn2 = max(n2)
    helper = maxn2 * Fr(EPS) ** 2 / 5
    rem = [list(c) for c in cols]
    order, rank, margin = [], 3, float("inf")
    left = [0, 1, 2]
    for k in range(3):
        nn = [dot(rem[j], rem[j]) for j in left]
        big = left[max(range(len(left)), key=lambda i: (nn[i], -i))]
        piv2 = dot(rem[big], rem[big])
        thr = helper * (5 - k)
        if rank == 3:
            if thr > 0:
                margin = min(margin, abs(float(mp.log(mp.mpf(piv2.numerator) / piv2.denominator / (mp.mpf(thr.numerator) / thr.denominator), 2))) if piv2 > 0 else 0.0)  # an exactly zero pivot: its computed value is rounding noise of the threshold's size
            if piv2 < thr:
                rank = k
        order.append(big)
        left.remove(big)
        if piv2 > 0:
            for j in left:
                f = dot(rem[j], rem[big]) / piv2
                rem[j] = [x - f * y for x, y in zip(rem[j], rem[big])]
    X = [Fr(0)] * 3
    if rank > 0:
        sel = order[:rank]
        G = [[dot(cols[i], cols[j]) for j in sel] for i in sel]
        b = [-sum(cols[i]) for i in sel]
        sol = solve3(G, b)
        if sol is None:  # Eigen's rule keeps a pivot that is exactly zero (0 < 0 is false on the zero matrix): no exact value
            return [np.nan] * 3, rank, np.nan, float("inf"), 0.0
        for i, v in zip(sel, sol):
            X[i] = v
    res2 = sum((sum(A[r][c] * X[c] for c in range(3)) + 1) ** 2 for r in range(5))
    # kappa from the eigenvalues of the exact Gram matrix
    G = [[dot(cols[i], cols[j]) for j in range(3)] for i in range(3)]
    kappa = float("inf")
    if rank == 3:
        s = max(abs(G[i][i]) for i in range(3))
        E, _ = mp.eigsy(mp.matrix([[mp.mpf(g.numerator) / g.denominator / (mp.mpf(s.numerator) / s.denominator) for g in row] for row in G]))
        lo, hi = min(E), max(E)
        kappa = float(mp.sqrt(hi / lo)) if lo > 0 else float("inf")
    return X, rank, float(mp.sqrt(mp.mpf(res2.numerator) / res2.denominator)), kappa, margin


# Campaign seed 930 (tests/gpu_fuzz.py, batch round 12, scan 13): the five neighbours, in search order, of the one plane record that
# differed from the oracle's, and the selected point as the oracle formed it and as the device formed it (x one float ulp apart:
# the two were given poses that differ by a matrix -> rotation vector -> matrix round trip).  The plane fit is the same for both.
SEED930_NB = [float.fromhex(v) for v in ['-0x1.68f2a80000000p-2', '0x1.dfdc9e0000000p+2', '0x1.ebfd140000000p+0', '-0x1.b99b680000000p-4', '0x1.e0029e0000000p+2', '0x1.ebb98c0000000p+0', '-0x1.67841a0000000p-2', '0x1.e0217e0000000p+2', '0x1.a842e00000000p+0', '-0x1.eab3800000000p-4', '0x1.dfe5ea0000000p+2', '0x1.a7ee100000000p+0', '-0x1.fea5300000000p-2', '0x1.e003100000000p+2', '0x1.ec84260000000p+0']]
SEED930_SEL = [[float.fromhex(v) for v in ['-0x1.eade100000000p-3', '0x1.e08b120000000p+2', '0x1.d635b00000000p+0']], [float.fromhex(v) for v in ['-0x1.eade120000000p-3', '0x1.e08b120000000p+2', '0x1.d635b00000000p+0']]]


def plane_pts(rng, n, offset, spread, noise=0.0):
    """5 float points on a random plane at distance `offset` from the origin"""
    out = []
    for _ in range(n):
        R = rot(rng)
        uv = rng.uniform(-1, 1, (5, 2)) * spread
        p = uv @ R[:2] + offset * R[2] + rng.normal(size=(5, 1)) * noise * R[2]
        out.append(f32(p))
    return out


def qr_families(rng):
    fam = {}
    fam["random_planes"] = [p for _ in range(550) for p in plane_pts(rng, 1, 10.0 ** rng.uniform(np.log10(0.5), np.log10(200)), rng.uniform(0.2, 2), 0.02)]
    it = []
    for _ in range(300):  # floors and walls: one exactly constant column
        p = f32(rng.uniform(-30, 30, (5, 3)))
        ax = rng.integers(3)
        p[:, ax] = f32(rng.uniform(-40, 40))
        it.append(p)
    fam["axis_aligned"] = it
    fam["near_origin"] = [p for _ in range(200) for p in plane_pts(rng, 1, 10.0 ** rng.uniform(-9, -3), rng.uniform(0.2, 2))]
    it = []
    for _ in range(120):
        a, d = rng.uniform(-20, 20, 3), rng.normal(size=3)
        if rng.random() < 0.5:  # exactly collinear in floats: multiples of one float vector
            v = f32(rng.uniform(-2, 2, 3))
            it.append(f32(np.outer(f32([1, 2, 3, 4, 8]), v)))
        else:
            it.append(f32(a + np.outer(rng.uniform(-1, 1, 5), d)))
    fam["collinear"] = it
    fam["coincident"] = [np.tile(f32(rng.uniform(-30, 30, 3)), (5, 1)) for _ in range(60)]
    it = []
    for _ in range(60):
        p = np.tile(f32(rng.uniform(-30, 30, 3)), (5, 1))
        p[rng.integers(5)] = f32(rng.uniform(-30, 30, 3))
        it.append(p)
    fam["four_plus_one"] = it
    fam["all_zero"] = [np.zeros((5, 3), np.float32), f32(np.zeros((5, 3)) * -1.0)]
    it = []
    for _ in range(650):  # two or three columns of exactly equal norm: permuted / sign-flipped copies of one column
        c = f32(rng.uniform(-10, 10, 5))
        p = np.empty((5, 3), np.float32)
        p[:, 0] = c
        p[:, 1] = rng.permutation(c) * rng.choice([-1, 1], 5)
        p[:, 2] = rng.permutation(c) * rng.choice([-1, 1], 5) if rng.random() < 0.5 else f32(rng.uniform(-10, 10, 5))
        it.append(p[:, rng.permutation(3)])
    fam["pivot_tie"] = it
    it = []
    for _ in range(200):  # col1 slightly longer than col2 but nearly parallel to col0: after the first reflector col2 leads
        c0 = rng.normal(size=5) * 10
        c1 = 0.8 * c0 + rng.normal(size=5) * rng.uniform(0.01, 0.5)
        c2 = rng.normal(size=5)
        c2 *= np.linalg.norm(c1) / np.linalg.norm(c2) * rng.uniform(0.5, 0.99)
        it.append(f32(np.stack([c0, c1, c2], 1)))
    fam["second_swap"] = it
    it = []
    for _ in range(200):  # near-parallel columns: the down-date cancels and the norm is recomputed
        c0 = rng.normal(size=5) * 10
        k = 10.0 ** rng.uniform(-7, -3)
        c1 = c0 * rng.uniform(0.3, 0.9) + rng.normal(size=5) * k
        c2 = c0 * rng.uniform(0.3, 0.9) + rng.normal(size=5) * (k if rng.random() < 0.5 else 1.0)
        it.append(f32(np.stack([c0, c1, c2], 1)))
    fam["downdate_recompute"] = it
    it = []
    for _ in range(350):  # voxel-filter output: a patch of a lattice plane, normal a small integer vector, on the 0.2 m lattice
        n = np.array([[1, 0, 1], [1, 1, 0], [0, 1, 1], [1, 1, 1], [1, -1, 0], [2, 1, 0], [0, 1, -2], [1, 2, 2]][rng.integers(8)])
        u = np.cross(n, [0, 0, 1] if n[0] or n[1] else [1, 0, 0])
        v = np.cross(n, u) // max(1, np.gcd.reduce(np.cross(n, u)))
        c = rng.integers(-150, 150, 3)
        while abs(int(n @ c)) < 10:
            c = rng.integers(-150, 150, 3)
        ij = rng.integers(-3, 4, (5, 2))
        while np.linalg.matrix_rank(np.c_[ij, np.ones(5)]) < 3:  # a patch, not a row of voxels
            ij = rng.integers(-3, 4, (5, 2))
        it.append(f32((c + ij[:, :1] * u + ij[:, 1:] * v) * 0.2))
    fam["lattice"] = it
    it = []
    for _ in range(40):  # a plane whose own largest residual is 0.2 +- k float ulps: (a,b,zt) (-a,-b,zt) (a,-b,zb) (-a,b,zb) (0,0,zm)
        # makes the Gram matrix diagonal, so X = (0, 0, -sum z / sum z^2) exactly, the plane is z = z0 = sum z^2 / sum z and the
        # lowest pair is z0 - zb off it; zb is moved ulp by ulp until that distance is the float-representable neighbour of 0.2
        h = float(f32(rng.uniform(2.2, 3.8)))
        u = (-1 + np.sqrt(1 + 4 * 0.2 * 4 / (5 * h))) / (8 / (5 * h))  # u + 4 u^2 / (5 h) = 0.2
        a, b = f32(rng.uniform(0.2, 2, 2))
        zt, zm, zb = f32(h + u), f32(h), f32(h - u)
        ulp = float(np.spacing(zb))

        def lowest(zb):
            z = [fr(zt), fr(zt), fr(zb), fr(zb), fr(zm)]
            return sum(v * v for v in z) / sum(z) - fr(zb)
        for _ in range(4):
            zb = ulps32(zb, int(round(float(lowest(zb) - Fr(1, 5)) / (1.1 * ulp))))
        for k in range(-4, 5):
            z = ulps32(zb, k)
            assert abs(float(lowest(z) - Fr(1, 5))) <= 8 * ulp, "gate_0p2: the lowest pair is not within ulps of the gate"
            it.append(f32([[a, b, zt], [-a, -b, zt], [a, -b, z], [-a, b, z], [0, 0, zm]]))
    fam["gate_0p2"] = it
    fam["seed930"] = [f32(SEED930_NB).reshape(5, 3)] * 2
    return fam


def plane_exact(p, sel, X, rank):
    """the plane model from the exact X: pa pb pc pd, the largest |residual| margin to 0.2 and proj of sel"""
    if rank == 0 or any(x != x for x in X) or sum(x * x for x in X) == 0:
        return [np.nan] * 4, np.nan, [np.nan] * 3
    n2 = sum(x * x for x in X)
    n = mp.sqrt(mp.mpf(n2.numerator) / n2.denominator)
    co = [mp.mpf(x.numerator) / x.denominator / n for x in X] + [1 / n]
    res = [abs(sum(co[c] * mp.mpf(float(row[c])) for c in range(3)) + co[3]) for row in p]
    margin = min(abs(r - mp.mpf("0.2")) for r in res)
    acc = all(r <= mp.mpf("0.2") for r in res)
    dist = sum(co[c] * mp.mpf(float(sel[c])) for c in range(3)) + co[3]
    proj = [mp.mpf(float(sel[c])) - dist * co[c] for c in range(3)]
    return [float(c) for c in co], (float(margin) if acc else -float(margin)), [float(v) for v in proj]


# ---------------------------------------------------------------------------------------------------------------------------
def line_families(rng):
    fam = {}
    it = []
    for _ in range(400):  # an edge: points along a direction with scatter
        a, d = rng.uniform(-40, 40, 3), rot(rng)[0]
        it.append(f32(a + np.outer(rng.uniform(-1, 1, 5), d) + rng.normal(size=(5, 3)) * 10.0 ** rng.uniform(-3, -0.5)))
    fam["edges"] = it
    fam["patches"] = [f32(rng.uniform(-40, 40, 3) + rng.normal(size=(5, 3)) * rng.uniform(0.1, 0.4)) for _ in range(300)]
    fam["lattice"] = [f32(rng.integers(-100, 100, 3) * 0.4 + rng.integers(-2, 3, (5, 3)) * 0.4) for _ in range(200)]
    fam["collinear"] = [f32(np.outer(f32([1, 2, 3, 4, 8]), f32(rng.uniform(-2, 2, 3)))) for _ in range(60)]
    fam["coincident"] = [np.tile(f32(rng.uniform(-30, 30, 3)), (5, 1)) for _ in range(40)] + [np.zeros((5, 3), np.float32)]
    it = []
    for _ in range(100):  # (+-a,0,0) (0,+-b,0) (0,0,0): a11 = 2a^2/5, a22 = 2b^2/5, a within ulps of sqrt(3) b
        b = f32(rng.uniform(0.1, 0.5))
        for k in range(-3, 4):
            a = ulps32(f32(np.sqrt(3.0) * float(b)), k)
            it.append(f32([[a, 0, 0], [-a, 0, 0], [0, b, 0], [0, -b, 0], [0, 0, 0]]))
    fam["gate3"] = it
    it = []
    for k in range(1, 201):  # x = (3,-3,0,0,0) s, y = (0,0,1,1,-2) s: covariance diag(18, 6, 0) s^2 / 5, ev2 = 3 ev1 exactly; every
        s = k / 64.0         # float operation before the division by 5 is exact, so about half of the items tie in floating point too
        p = np.zeros((5, 3))
        p[:, 0], p[:, 1] = np.array([3, -3, 0, 0, 0]) * s, np.array([0, 0, 1, 1, -2]) * s
        it.append(f32(p[:, rng.permutation(3)]))
    fam["gate3_tie"] = it
    return fam


def line_exact(p):
    P = [[fr(v) for v in row] for row in p]
    c = [sum(P[j][k] for j in range(5)) / 5 for k in range(3)]
    D = [[P[j][k] - c[k] for k in range(3)] for j in range(5)]
    S = [[sum(D[j][a] * D[j][b] for j in range(5)) / 5 for b in range(3)] for a in range(3)]
    Sm = mp.matrix([[mp.mpf(v.numerator) / v.denominator for v in row] for row in S])
    s = max(abs(Sm[i, j]) for i in range(3) for j in range(3))
    if s == 0:
        return [float(v) for v in c], [0.0] * 3, [np.nan] * 3, 0.0
    E, Q = mp.eigsy(Sm / s)
    o = sorted(range(3), key=lambda i: E[i])
    ev = [E[i] * s for i in o]
    return [float(v) for v in c], [float(v) for v in ev], [float(Q[r, o[2]]) for r in range(3)], float(s)


def ops_inputs(rng):
    a = rng.integers(0, 2 ** 63, 1000, dtype=np.int64).view(np.float64)
    b = rng.integers(-2 ** 63, 2 ** 63 - 1, 1000, dtype=np.int64).view(np.float64)
    pairs = [np.stack([a, b], 1)]
    den = rng.integers(1, 2 ** 52, 500, dtype=np.int64).view(np.float64)
    pairs.append(np.stack([den, rng.uniform(0.1, 10, 500)], 1))
    pairs.append(np.stack([rng.uniform(0.1, 10, 500), den[::-1] * 2.0 ** 1000], 1))
    r = rng.uniform(0.5, 200, (1000, 3))
    ss = (r * r).sum(1)  # sums of squares of lidar-range doubles
    pairs.append(np.stack([ss, r[:, 0]], 1))
    k = rng.integers(1, 2 ** 26, 600).astype(np.float64)
    h = 1.0 + k * 2.0 ** -27  # (1 + k 2^-27)^2 needs 55 bits: its double neighbours are near-halfway cases for sqrt
    sq = h * h
    pairs.append(np.stack([np.concatenate([ulps64(sq, -1), sq, ulps64(sq, 1)]), np.concatenate([h, h, h])], 1))
    p64 = np.concatenate(pairs)
    a = rng.integers(0, 2 ** 31, 1000, dtype=np.int64).astype(np.int32).view(np.float32)
    b = rng.integers(-2 ** 31, 2 ** 31 - 1, 1000, dtype=np.int64).astype(np.int32).view(np.float32)
    q = [np.stack([a, b], 1)]
    den = rng.integers(1, 2 ** 23, 500, dtype=np.int64).astype(np.int32).view(np.float32)
    q.append(np.stack([den, f32(rng.uniform(0.1, 10, 500))], 1))
    k = rng.integers(1, 2 ** 11, 1500).astype(np.float32)
    h = f32(1.0) + k * f32(2.0 ** -12)
    sq = h * h
    q.append(np.stack([np.concatenate([ulps32(sq, -1), sq, ulps32(sq, 1)]), np.concatenate([h, h, h])], 1))
    r = f32(rng.uniform(0.5, 200, (1000, 3)))
    q.append(np.stack([(r * r).sum(1), r[:, 0]], 1))
    return p64, np.concatenate(q).astype(np.float32)


def flatten(fam, width, dtype):
    names = list(fam)
    items = np.concatenate([np.asarray(fam[n], dtype).reshape(-1, width) for n in names])
    idx = np.concatenate([np.full(len(fam[n]), i, np.int16) for i, n in enumerate(names)])
    return names, items, idx


def check_share(names, idx, undec, threshold_families, what):
    for i, n in enumerate(names):
        m = idx == i
        if n in threshold_families or not m.any():
            continue
        share = undec[m].mean()
        assert share <= 1e-3, "%s family %s: %.2f %% of the items are undecidable" % (what, n, 100 * share)


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 20261016
    rng = np.random.default_rng(seed)
    out = {}
    # eig3
    names, items, idx = flatten(eig3_families(rng), 6, np.float64)
    out.update(eig3_families=np.array(names), eig3_in=items, eig3_fam=idx,
               eig3_ev=np.array([[float(v) for v in eig_exact(m)[0]] for m in items]))
    # qr
    names, items, idx = flatten(qr_families(rng), 15, np.float64)
    ex = [qr_exact(a.reshape(5, 3)) for a in items]
    assert np.array_equal(items.astype(np.float32).astype(np.float64), items)
    out.update(qr_families=np.array(names), qr_in=items.astype(np.float32), qr_fam=idx, qr_x=np.array([[float(v) for v in e[0]] for e in ex]),
               qr_rank=np.array([e[1] for e in ex], np.int8), qr_resid=np.array([e[2] for e in ex]),
               qr_kappa=np.array([e[3] for e in ex]), qr_rank_margin=np.array([e[4] for e in ex]))
    rank_fams = {"pivot_tie", "collinear", "coincident", "four_plus_one", "all_zero"}  # built on, or holding items on, a rank threshold
    check_share(names, idx, out["qr_rank_margin"] <= np.log2(RANK_BAND), rank_fams, "qr rank")
    # plane model: the qr items as float points + a selected point near their centroid
    pts = items.astype(np.float32)
    sel = f32(pts.reshape(-1, 5, 3).mean(1) + rng.normal(size=(len(pts), 3)) * 0.3)
    sel[idx == names.index("seed930")] = f32(SEED930_SEL)
    pm = [plane_exact(p.reshape(5, 3), s, e[0], e[1]) for p, s, e in zip(pts, sel, ex)]
    coef = np.array([m[0] for m in pm])
    out.update(plane_sel=sel, plane_coef=coef, plane_margin=np.array([m[1] for m in pm]),
               plane_proj=np.array([m[2] for m in pm]))
    with np.errstate(invalid="ignore"):
        band = (PLANE_BAND * EPSF + QR_BAND * EPS * out["qr_kappa"] ** 2) * (np.abs(pts).max(1) + 1)
        undec = ~(np.abs(out["plane_margin"]) > band) | (out["qr_rank"] < 3) | (out["qr_rank_margin"] <= np.log2(RANK_BAND))
    out["plane_undecidable"] = undec
    g = idx == names.index("gate_0p2")
    assert np.abs(out["plane_margin"][g]).max() <= 8 * 2.4e-7, "gate_0p2 is not at the few-ulp level"
    # the 0.2 m gate: besides the family on the gate, the families ill-conditioned by construction (kappa^2 eps reaches the band)
    check_share(names, idx, undec, rank_fams | {"gate_0p2", "near_origin", "downdate_recompute", "second_swap"}, "plane gate")
    # line model
    names, items, idx = flatten(line_families(rng), 15, np.float32)
    le = [line_exact(p.reshape(5, 3)) for p in items]
    ev = np.array([e[1] for e in le])
    out.update(line_families=np.array(names), line_in=items, line_fam=idx, line_cen=np.array([e[0] for e in le]), line_ev=ev,
               line_dir=np.array([e[2] for e in le]), line_scale=np.array([e[3] for e in le]))
    pmax = np.abs(items).max(1).astype(np.float64)
    undec = np.abs(ev[:, 2] - 3 * ev[:, 1]) <= LINE_BAND * (EPSF * (out["line_scale"] + pmax * np.sqrt(out["line_scale"])) + (EPSF * pmax) ** 2)
    out["line_undecidable"] = undec
    check_share(names, idx, undec, {"gate3", "gate3_tie", "coincident", "collinear"}, "line gate")
    out["ops64_in"], out["ops32_in"] = ops_inputs(rng)
    out.update(bands=np.array([LINE_BAND, PLANE_BAND, QR_BAND, RANK_BAND]), seed=np.array(seed))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "modelfit_kat.npz" if len(sys.argv) < 3 else sys.argv[2])
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: len(v) for k, v in out.items() if k.endswith("_in")})


if __name__ == "__main__":
    main()
