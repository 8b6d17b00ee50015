"""Writes tests/golden/gicp_kat.npz: known answers for the pieces of the GICP (csrc/gicp.hip, oracle/gicp.cpp), computed from the
operations' DEFINITIONS with mpmath at 80 digits on the exact rationals of the float / double inputs -- never from the project's
formulas.  Data only.  Rerun: python tests/golden/make_gicp_kat.py (byte-identical output; every cap below is asserted).

  objective   f(x) = 1/m sum res' M res, res = Rz(psi) Ry(theta) Rx(phi) p + t - q over the kept correspondences.  The exact sum is
              formed once per list as the tensor S = sum M (x) z z', z = (p, 1, q), so that f = 1/m <B' S B>, B = [R | t | -I]: an
              exact rearrangement of the definition.  The gradient is the central difference of that f with step 1e-24; no
              derivative-of-rotation formula appears here (the entries of dR used by the visibility assertion are central
              differences of R itself).
  quadratic   the real roots of a x^2 + b x + c from the exact discriminant: count, ascending order, values
  interpolate the minimiser over the closed interval of the cubic through (f, f') at both ends (coefficients from the four
              Hermite conditions by a linear solve), or of the quadratic through (fa, fpa, fb) when fpb is NaN; candidates are the
              two ends and the interior stationary points; mapped back to alpha.  Undecidable: the two best candidates' values
              closer than 64 * 2^-52 * max |coefficient| (at most 1 % per family).
  neighbours  the 20 smallest EXACT squared distances, ties to the lower index.  Undecidable: the exact 20th and 21st closer than the
              float rounding 4 * 2^-24 * d of (dx^2 + dy^2) + dz^2 (a true tie between exact float distances, or between two copies of
              one point, is decided by the index); at most 1 % per family
  covariance  I - (1 - 1e-3) u0 u0' from the exact covariance of 20 points (mpmath's symmetric eigen-solver at 80 digits)
  corr / maha the exact 1-NN of T p (real arithmetic on the float entries of T), the gate d < gate^2, M = (R C1 R' + C2)^-1 exactly
  state       the entries of Rz Ry Rx of the FLOAT-rounded angles, and x itself for the recovery
  round       two problems (inputs only; the properties are checked against the exact objective at test time)
"""
import os
import sys
import zipfile
from fractions import Fraction

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gicp_checks as K  # noqa: E402  (the units; nothing measured)

mp.mp.dps = 80
STEP = mp.mpf(10) ** -24
M_ = lambda v: mp.mpf(float(v))                                   # the exact rational of a float / double


def rot(phi, th, psi):
    c, s = mp.cos, mp.sin
    Rx = mp.matrix([[1, 0, 0], [0, c(phi), -s(phi)], [0, s(phi), c(phi)]])
    Ry = mp.matrix([[c(th), 0, s(th)], [0, 1, 0], [-s(th), 0, c(th)]])
    Rz = mp.matrix([[c(psi), -s(psi), 0], [s(psi), c(psi), 0], [0, 0, 1]])
    return Rz * Ry * Rx


# ---- objective ----------------------------------------------------------------------------------------------------------------
def planar_cov(rng, n):
    """GICP covariances I - (1 - 1e-3) u u' for random unit normals u (inputs of the objective, in doubles)"""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return np.eye(3)[None] - (1 - 1e-3) * u[:, :, None] * u[:, None, :]


def eval_inputs(rng):
    n = K.EVAL_N
    src = rng.uniform(-8, 8, (n, 3)).astype(np.float32)
    tgt = (rng.uniform(-8, 8, (n, 3))).astype(np.float32)
    corr = rng.permutation(n).astype(np.int32)
    Rr = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    C1, C2 = planar_cov(rng, n), planar_cov(rng, n)
    maha = np.linalg.inv(Rr @ C1 @ Rr.T + C2[corr])
    return src, tgt, corr, maha


def point_tensor(p, q, M):
    z = np.array([M_(p[0]), M_(p[1]), M_(p[2]), mp.mpf(1), M_(q[0]), M_(q[1]), M_(q[2])], dtype=object)
    Mm = np.array([M_(v) for v in M.reshape(9)], dtype=object).reshape(3, 3)
    return np.multiply.outer(Mm, np.multiply.outer(z, z))          # [i, k, a, b]


def f_exact(S, m, x):
    R = rot(x[3], x[4], x[5])
    B = np.array([[R[i, 0], R[i, 1], R[i, 2], x[i]] + [mp.mpf(-1) if j == i else mp.mpf(0) for j in range(3)] for i in range(3)], dtype=object)
    G = np.tensordot(B, S, axes=([0, 1], [0, 2]))                  # [k, b]
    return (G * B).sum() / m


def grad_exact(S, m, x):
    g = []
    for k in range(6):
        xp, xm = list(x), list(x)
        xp[k] += STEP
        xm[k] -= STEP
        g.append((f_exact(S, m, xp) - f_exact(S, m, xm)) / (2 * STEP))
    return g


def make_eval(rng):
    src, tgt, corr, maha = eval_inputs(rng)
    per = [point_tensor(src[i], tgt[corr[i]], maha[i]) for i in range(K.EVAL_N)]
    lists = K.eval_lists()
    states = K.EVAL_STATES
    f = np.zeros((len(lists), len(states)))
    g = np.zeros((len(lists), len(states), 6))
    for li, (n, holes) in enumerate(lists):
        keep = np.ones(n, bool)
        keep[holes] = False
        S = sum(per[i] for i in np.flatnonzero(keep))
        m = int(keep.sum())
        for si, x in enumerate(states):
            xe = [M_(v) for v in x]
            f[li, si] = float(f_exact(S, m, xe))
            g[li, si] = [float(v) for v in grad_exact(S, m, xe)]
    out = dict(ev_src=src, ev_tgt=tgt, ev_corr=corr, ev_maha=maha.reshape(-1, 9), ev_f=f, ev_g=g)
    # every entry of dR/dphi, dR/dtheta, dR/dpsi that is not identically zero moves some gradient component of some O(1)-angle
    # item by more than 100 units: a wrong entry cannot hide.  dR by central differences of R; G = df/dR in doubles (a magnitude).
    u = K.eval_units(out)
    seen = np.zeros((3, 3, 3))
    for si in K.EVAL_O1:
        x = states[si]
        xe = [M_(v) for v in x]
        for k in range(3):
            xp, xm = list(xe), list(xe)
            xp[3 + k] += STEP
            xm[3 + k] -= STEP
            dR = (rot(*xp[3:]) - rot(*xm[3:])) / (2 * STEP)
            dR = np.array([[float(dR[i, j]) for j in range(3)] for i in range(3)])
            for li, (n, holes) in enumerate(lists):
                G = K.eval_dfdR(out, li, x)
                seen[k] = np.maximum(seen[k], np.abs(dR * G) / u["u_g"][li, si, 3 + k])
    live = np.ones((3, 3, 3), bool)
    live[0, :, 0] = False                                          # Rx leaves column 0 of R alone: dR/dphi has none there
    live[2, 2, :] = False                                          # Rz leaves row 2 alone
    assert (seen[live] > 100).all(), seen
    assert (seen[~live] < 1e-12).all()
    out["ev_seen"] = seen
    return out


# ---- solve_quadratic ----------------------------------------------------------------------------------------------------------
def quad_families(rng):
    fam = {}
    mags = [1e-12, 1e-6, 1e-3, 1.0, 1e3, 1e6]
    two = []
    for s in mags:
        for _ in range(12):
            r1, r2 = rng.uniform(0.1, 3) * rng.choice([-1, 1]), rng.uniform(4, 30) * rng.choice([-1, 1])
            a = rng.uniform(0.5, 2) * rng.choice([-1, 1]) * s
            two.append((a, -a * (r1 + r2) * np.sqrt(s), a * r1 * r2 * s))
    fam["q_two_roots"] = two
    fam["q_no_root"] = [(a * s, b * s, (b * b / (4 * a)) * s * rng.uniform(1.5, 9)) for s in mags for a, b in
                        [(rng.uniform(0.5, 2) * rng.choice([-1, 1]), rng.uniform(-3, 3)) for _ in range(4)]]
    fam["q_disc_zero"] = [(float(a) * s, 2.0 * a * k * s, float(a) * k * k * s) for s in (2.0 ** -30, 1.0, 2.0 ** 20) for a in (1, -1, 4) for k in (1, -3, 5, 0.25)]
    fam["q_linear"] = [(0.0, rng.uniform(0.5, 2) * rng.choice([-1, 1]) * s, rng.uniform(-3, 3) * s2) for s in mags for s2 in (1e-6, 1.0, 1e6)]
    fam["q_both_zero"] = [(0.0, 0.0, c) for c in (0.0, 1.0, -2.5, 1e-12, 1e6)]
    fam["q_b_zero"] = [(rng.uniform(0.5, 2) * sg * s, 0.0, -rng.uniform(0.5, 2) * sg * s2) for s in mags for s2 in (1e-6, 1.0, 1e6) for sg in (1, -1)]
    return fam


def quad_exact(a, b, c):
    a, b, c = M_(a), M_(b), M_(c)
    if a == 0:
        return (0, 0, 0) if b == 0 else (1, -c / b, 0)
    disc = b * b - 4 * a * c                                       # exact: products of doubles fit 80 digits
    if disc < 0:
        return 0, 0, 0
    r = mp.sqrt(disc)
    x = sorted([(-b - r) / (2 * a), (-b + r) / (2 * a)])
    return 2, x[0], x[1]


# ---- interpolate ----------------------------------------------------------------------------------------------------------------
def interp_exact(it):
    a, fa, fpa, b, fb, fpb, xmin, xmax = it
    cubic = np.isfinite(fpb)
    a, fa, fpa, b, fb, xmin, xmax = (M_(v) for v in (a, fa, fpa, b, fb, xmin, xmax))
    h = b - a
    lo, hi = sorted([(xmin - a) / h, (xmax - a) / h])
    f0, fp0, f1 = fa, fpa * h, fb
    if cubic:
        fp1 = M_(fpb) * h
        # p(0) = f0, p'(0) = fp0, p(1) = f1, p'(1) = fp1
        c = mp.lu_solve(mp.matrix([[1, 0, 0, 0], [0, 1, 0, 0], [1, 1, 1, 1], [0, 1, 2, 3]]), mp.matrix([f0, fp0, f1, fp1]))
        c = [c[i] for i in range(4)]
    else:
        c = mp.lu_solve(mp.matrix([[1, 0, 0], [0, 1, 0], [1, 1, 1]]), mp.matrix([f0, fp0, f1]))
        c = [c[i] for i in range(3)] + [mp.mpf(0)]
    p = lambda z: c[0] + z * (c[1] + z * (c[2] + z * c[3]))
    cnt, s0, s1 = quad_exact_mp(3 * c[3], 2 * c[2], c[1])
    cand = [lo, hi] + [z for z in (s0, s1)[:cnt] if lo < z < hi]
    vals = [p(z) for z in cand]
    order = sorted(range(len(cand)), key=lambda i: (vals[i], i))
    best = cand[order[0]]
    band = 64 * mp.mpf(2) ** -52 * max(abs(v) for v in c)
    near = [cand[i] for i in order if vals[i] - vals[order[0]] < band and cand[i] != best]
    other = near[0] if near else best
    d2 = abs(2 * c[2] + 6 * c[3] * best)                            # |p''| at the minimiser (used by the unit of an interior one)
    interior = lo < best < hi
    return (float(a + best * h), float(a + other * h), bool(near), float(best), float(d2), bool(interior), float(max(abs(v) for v in c)))


def quad_exact_mp(a, b, c):
    if a == 0:
        return (0, 0, 0) if b == 0 else (1, -c / b, 0)
    disc = b * b - 4 * a * c
    if disc < 0:
        return 0, 0, 0
    r = mp.sqrt(disc)
    return 2, (-b - r) / (2 * a), (-b + r) / (2 * a)


def interp_families(rng):
    """items (a, fa, fpa, b, fb, fpb, xmin, xmax) as the line search forms them and beyond"""
    fam = {k: [] for k in ("i_lower_end", "i_upper_end", "i_root1", "i_root2", "i_no_stationary", "i_disc_zero", "i_linear", "i_flat",
                           "i_b_zero", "i_reversed", "i_quad_neg", "i_quad_pos_in", "i_quad_pos_out", "i_magnitudes")}
    nan = float("nan")

    def hermite(c0, c1, c2, c3, a, b):
        """(fa, fpa, fb, fpb) of the cubic c0 + c1 z + c2 z^2 + c3 z^3 in z = (alpha - a) / (b - a)"""
        h = b - a
        return c0, c1 / h, c0 + c1 + c2 + c3, (c1 + 2 * c2 + 3 * c3) / h
    for _ in range(24):
        a, b = rng.uniform(-1, 1), rng.uniform(2, 5)
        # p' = 3 c3 (z - r1)(z - r2), c3 > 0: local max at r1 < local min at r2
        c3 = rng.uniform(0.5, 2)
        mk = lambda r1, r2: hermite(rng.uniform(-1, 1), 3 * c3 * r1 * r2, -1.5 * c3 * (r1 + r2), c3, a, b)
        iv = lambda zl, zh: (a + zl * (b - a), a + zh * (b - a))
        fa, fpa, fb, fpb = mk(-2.0, -1.0)                          # increasing on the interval: minimum at the lower end
        fam["i_lower_end"].append((a, fa, fpa, b, fb, fpb, *iv(0.1, 0.9)))
        fa, fpa, fb, fpb = mk(-1.0, 3.0)                           # decreasing on it: the upper end
        fam["i_upper_end"].append((a, fa, fpa, b, fb, fpb, *iv(0.1, 0.9)))
        r2 = rng.uniform(0.3, 0.7)
        fa, fpa, fb, fpb = mk(-1.0, r2)                            # local minimum inside: the larger root (c3 > 0)
        fam["i_root2"].append((a, fa, fpa, b, fb, fpb, *iv(0.05, 0.95)))
        c3 = -c3                                                   # c3 < 0: the local minimum is the smaller root
        fa, fpa, fb, fpb = mk(r2, 2.0)
        fam["i_root1"].append((a, fa, fpa, b, fb, fpb, *iv(0.05, 0.95)))
        c3 = abs(c3)
        sg = rng.choice([-1, 1])
        fa, fpa, fb, fpb = hermite(0.3, sg * rng.uniform(0.5, 2), rng.uniform(-0.2, 0.2), sg * c3, a, b)                 # p' has no real root
        fam["i_no_stationary"].append((a, fa, fpa, b, fb, fpb, *iv(0.1, 0.9)))
        fa, fpa, fb, fpb = hermite(0.25, rng.uniform(-2, 2), rng.uniform(-2, 2), 0.0, a, b)                             # a parabola: p' linear
        fam["i_linear"].append((a, fa, fpa, b, fb, fpb, *iv(0.05, 0.95)))
        fa, fpa, fb, fpb = mk(-1.0, r2)
        fam["i_reversed"].append((b, fb, fpb, a, fa, fpa, *iv(0.95, 0.05)))                                             # a > b and xmin > xmax
        # quadratics (fpb = NaN): curvature c = 2 (f1 - f0 - fp0)
        fp0, cn = rng.uniform(0.2, 1) * rng.choice([-1, 1]), -rng.uniform(0.5, 3)
        fam["i_quad_neg"].append((a, 1.0, fp0 / (b - a), b, 1.0 + fp0 + cn / 2, nan, *iv(0.1, 0.9)))
        z = rng.uniform(0.2, 0.8)
        cq = rng.uniform(0.5, 3)
        fam["i_quad_pos_in"].append((a, 2.0, -cq * z / (b - a), b, 2.0 - cq * z + cq / 2, nan, *iv(0.05, 0.95)))
        zo = rng.choice([-0.5, 1.6])
        fam["i_quad_pos_out"].append((a, 2.0, -cq * zo / (b - a), b, 2.0 - cq * zo + cq / 2, nan, *iv(0.05, 0.95)))
        s = 10.0 ** rng.integers(-12, 7)
        fa, fpa, fb, fpb = mk(-1.0, r2)
        fam["i_magnitudes"].append((a * s, fa * s, fpa, b * s, fb * s, fpb, *(v * s for v in iv(0.05, 0.95))))
    # p' = 3 (z - r)^2 in small dyadic numbers: its discriminant is exactly 0 in doubles as well
    for r in (0.25, 0.5, 0.75, -0.5):
        for a, b in ((0.0, 1.0), (1.0, 3.0)):
            fam["i_disc_zero"].append((a, *hermite(1.0, 3 * r * r, -3 * r, 1.0, a, b)[:2], b, *hermite(1.0, 3 * r * r, -3 * r, 1.0, a, b)[2:], a + 0.125 * (b - a), a + 0.875 * (b - a)))
    # p' = 3 c3 (z^2 - 1/4) in dyadic numbers: the middle coefficient of p' is exactly 0 in doubles as well, roots -1/2 and 1/2
    for c3 in (1.0, 2.0, -1.0, -4.0):
        for a, b in ((0.0, 1.0), (1.0, 3.0)):
            fa, fpa, fb, fpb = hermite(0.5, -0.75 * c3, 0.0, c3, a, b)
            fam["i_b_zero"].append((a, fa, fpa, b, fb, fpb, a - 0.875 * (b - a), a + 0.875 * (b - a)))
    for v in (0.0, 1.5, -2.0):                                    # a constant: both coefficients of p' are 0
        fam["i_flat"].append((0.0, v, 0.0, 2.0, v, 0.0, 0.25, 1.5))
    return {k: [tuple(float(x) for x in it) for it in v] for k, v in fam.items()}


# ---- state ----------------------------------------------------------------------------------------------------------------------
def state_cases(rng):
    pi32 = float(np.float32(np.pi))
    xs = [(0, 0, 0, 0.0, 0.0, 0.0), (0, 0, 0, -0.0, -0.0, -0.0), (1, -2, 3, 1e-8, -1e-8, 1e-8), (0.05, 0, 5, -1e-8, 1e-8, -1e-8),
          (0, 0, 0, pi32, 0.3, -pi32), (1, 1, 1, -pi32, -0.3, pi32), (5, -5, 0.05, 0.3, 1.5, -0.4), (0, 0, 0, -2.5, -1.5, 2.8)]
    for sp in (1, -1):
        for st in (1, -1):
            for ss in (1, -1):
                for mag in (0.7, 2.4):
                    xs.append((rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-5, 5), sp * mag, st * rng.uniform(0.1, 1.5), ss * (3.1 - mag)))
    return np.array(xs, dtype=np.float64)


def state_exact(x):
    a = [M_(np.float32(v)) for v in x[3:]]
    R = rot(*a)
    return np.array([[float(R[i, j]) for j in range(3)] for i in range(3)])


# ---- one round -------------------------------------------------------------------------------------------------------------------
def round_problems(rng):
    """inputs only: a cloud against a displaced copy of itself (300 points, no gate; 513 points, 2 m gate dropping some)"""
    out = {}
    for name, n, gate in (("r300", 300, 0.0), ("r513", 513, 2.0)):
        tgt = np.concatenate([rng.uniform(-6, 6, (n, 2)), rng.normal(0, 0.05, (n, 1))], 1)
        tgt[n // 2:, [0, 2]] = tgt[n // 2:, [2, 0]]                 # two walls
        tgt = tgt.astype(np.float32)
        Rd = np.array(state_exact((0, 0, 0, 0.02, -0.015, 0.03)))
        src = ((tgt.astype(np.float64) - [0.08, -0.05, 0.06]) @ Rd).astype(np.float32)
        if gate:                                                   # some source points further than the gate from everything
            src[::17] += np.float32(40.0)
        out[name + "_src"], out[name + "_tgt"], out[name + "_gate"] = src, tgt, np.float64(gate)
    return out


# ---- neighbours ----------------------------------------------------------------------------------------------------------------
F_ = lambda v: Fraction(float(v))                                  # the exact rational of a float / double
BAND_D = 4 * 2.0 ** -24                                            # float rounding of (dx^2 + dy^2) + dz^2, relative to d


def exact_nearest(pts, q, k):
    """the k + 1 (at most) points nearest to q (three Fractions) by EXACT squared distance, ties to the lower index -> [(d, index)].
    Doubles only pre-select the candidates (differences of floats are exact in doubles; the margin is 1e7 x their rounding)."""
    d64 = ((pts.astype(np.float64) - np.array([float(v) for v in q])) ** 2).sum(1)
    kk = min(k + 1, len(pts))
    thr = np.partition(d64, kk - 1)[kk - 1]
    cand = np.flatnonzero(d64 <= thr * (1 + 1e-9) + 1e-12)
    ex = sorted((sum((F_(pts[j, a]) - q[a]) ** 2 for a in range(3)), int(j)) for j in cand)
    return ex[:kk]


def float_distance_is_exact(p, q, d):
    dx, dy, dz = (np.float32(p[a]) - np.float32(q[a]) for a in range(3))
    return F_((dx * dx + dy * dy) + dz * dz) == d


def nn_families(rng):
    fam = {}
    for n in (20, 21, 255, 256, 257, 1023, 1024, 1025, 1100):      # GK, the 256-lane blocks, the 1024-point tiles
        p = rng.uniform(-4, 4, (n, 3))
        p[:, 2] *= 0.05
        fam["nn_random_%d" % n] = p
    cell = rng.permutation(8 * 8 * 5)[:300]                        # coordinates in multiples of 1/8: every distance exact in float,
    fam["nn_lattice"] = np.stack([cell % 8, (cell // 8) % 8, cell // 64], 1) / 8.0    # ties are true ties, decided by the index
    d = rng.uniform(-1, 1, (85, 3))
    d[10:35] = d[10]                                               # 25 copies of one point: more than GK at distance 0
    d[50:52] = d[50]
    fam["nn_duplicates"] = d
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 0.05
    fam["nn_far_60m"] = g + rng.normal(0, 0.004, g.shape) + [40.0, -40.0, 20.0]       # 60 m from the origin, 5 cm spacing
    return {k: v.astype(np.float32) for k, v in fam.items()}


def make_neighbours(rng):
    fam = nn_families(rng)
    ids, und, d20, off = [], [], [], [0]
    for name, pts in fam.items():
        u_fam = []
        for i in range(len(pts)):
            top = exact_nearest(pts, [F_(v) for v in pts[i]], 20)
            ids.append([j for _, j in top[:20]])
            d20.append(float(top[19][0]))
            u = False
            if len(top) > 20:
                a, b = top[19], top[20]
                if a[0] == b[0]:           # a true tie: the index decides it iff both float distances are exact, or the two are one point twice
                    u = not ((pts[a[1]] == pts[b[1]]).all() or
                             (float_distance_is_exact(pts[a[1]], pts[i], a[0]) and float_distance_is_exact(pts[b[1]], pts[i], b[0])))
                else:
                    u = float(b[0] - a[0]) < BAND_D * float(b[0])
            u_fam.append(u)
        assert np.mean(u_fam) <= 0.01, (name, np.mean(u_fam))      # the cap: at most 1 % of a family undecidable
        und += u_fam
        off.append(off[-1] + len(pts))
    lat = fam["nn_lattice"].astype(np.float64) * 8
    assert (lat == np.round(lat)).all()
    return dict(nn_names=np.array(list(fam)), nn_off=np.array(off, np.int32), nn_pts=np.concatenate(list(fam.values())),
                nn_ids=np.array(ids, np.int16), nn_undecidable=np.array(und), nn_d20=np.array(d20))


# ---- covariance ----------------------------------------------------------------------------------------------------------------
def cov_families(rng):
    """clouds of exactly 20 points: every point's 20 neighbours are the whole cloud, in 20 different orders.  No cloud has
    coincident or exactly collinear points -- u0 is undefined there -- (asserted: the middle eigenvalue is positive)."""
    def patch(noise, dist, ext=(1.0, 1.0)):
        Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        local = np.stack([rng.uniform(-0.5, 0.5, 20) * ext[0], rng.uniform(-0.5, 0.5, 20) * ext[1], rng.normal(0, noise, 20)], 1)
        c = rng.normal(size=3)
        return (local @ Q.T + c * (dist / np.linalg.norm(c))).astype(np.float32)
    fam = {}
    for noise in (1e-2, 1e-3, 1e-4):
        for dist in (0, 10, 60):
            fam["cov_plane_%g_%dm" % (noise, dist)] = [patch(noise, dist) for _ in range(8)]
    fam["cov_edge"] = [patch(3e-3, dist, ext=(1.0, 0.03)) for dist in (0, 0, 0, 0, 2, 2, 2, 10, 10, 10, 60, 60)]   # lambda_1 - lambda_0 about 7e-5
    return fam


def cov_exact(P):
    """I - (1 - 1e-3) u0 u0', u0 the eigenvector of the smallest eigenvalue of the exact covariance of the 20 points; and the gap"""
    X = [[F_(v) for v in p] for p in P]
    mean = [sum(x[a] for x in X) / 20 for a in range(3)]
    C = [[sum(x[a] * x[b] for x in X) / 20 - mean[a] * mean[b] for b in range(3)] for a in range(3)]
    E, V = mp.eigsy(mp.matrix([[mp.mpf(c.numerator) / c.denominator for c in row] for row in C]))
    order = sorted(range(3), key=lambda i: E[i])
    u0 = [V[a, order[0]] for a in range(3)]
    assert E[order[1]] > 0
    keep = 1 - mp.mpf("1e-3")
    return [float((1 if a == b else 0) - keep * u0[a] * u0[b]) for a in range(3) for b in range(3)], float(E[order[1]] - E[order[0]])


def make_cov(rng):
    fam = cov_families(rng)
    items = [(k, n, P) for k, n in enumerate(fam) for P in fam[n]]
    ex = [cov_exact(P) for _, _, P in items]
    out = dict(cv_names=np.array(list(fam)), cv_fam=np.array([k for k, _, _ in items], np.int16), cv_pts=np.stack([P for _, _, P in items]),
               cv_C=np.array([e[0] for e in ex]), cv_gap=np.array([e[1] for e in ex]))
    out["cv_spectrum_only"] = K.cov_first_order(out) > K.COV_BAND
    plane = np.array([not n.startswith("cov_edge") for _, n, _ in items])
    assert out["cv_spectrum_only"][plane].mean() <= 0.01           # the cap on the non-edge families
    assert 0 < out["cv_spectrum_only"][~plane].sum() < (~plane).sum()
    return out


# ---- correspondence and Mahalanobis --------------------------------------------------------------------------------------------
def normals_cov(rng, n):
    return planar_cov(rng, n)


def make_corr(rng):
    f32 = np.float32
    tgt_all, src_all = rng.uniform(-3, 3, (1025, 3)).astype(f32), rng.uniform(-3, 3, (1025, 3)).astype(f32)

    def Tof(angles, t):
        T = np.eye(4, dtype=f32)
        T[:3, :3] = K.rotation([0, 0, 0, *angles]).astype(f32)
        T[:3, 3] = t
        return T
    I4, T1, Ts = np.eye(4, dtype=f32), Tof((0.9, -0.7, 1.1), (0.3, -0.2, 0.1)), Tof((4e-3, -3e-3, 2e-3), (0.03, -0.02, 0.01))
    grid = (np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3) * 2.0).astype(f32)
    dirs = rng.normal(size=(64, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    sides = (grid + dirs * 0.5 * (1 + 1e-3 * np.where(np.arange(64) % 2, 1, -1))[:, None]).astype(f32)   # about 1e-3 either side of a 0.5 m gate
    lat = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32)       # spacing 1, offsets in eighths
    lat_src = np.concatenate([lat + f32([0.375, 0.5, 0]), lat + f32([0.375, 0.375, 0]), lat + f32([0.5, 0.5, 0])])   # d = 25/64 (= gate^2), 18/64, 32/64
    # (name, src, tgt, T, gate, exact float arithmetic by construction)
    cases = [("c_1x1_identity", src_all[:1], tgt_all[:1], I4, 0.0, False), ("c_255x1024_identity", src_all[:255], tgt_all[:1024], I4, 0.0, False),
             ("c_256x1_1rad", src_all[:256], tgt_all[:1], T1, 0.0, False), ("c_257x1025_small", src_all[:257], tgt_all, Ts, 0.0, False),
             ("c_1025x1025_1rad_gated", src_all, tgt_all, T1, 0.5, False), ("c_gate_sides", sides, grid, I4, 0.5, False),
             ("c_gate_lattice", lat_src, lat, I4, 0.625, True)]
    out = {k: [] for k in ("src", "tgt", "C1", "C2", "T", "gate2", "corr", "corr2", "M", "und", "ns", "nt")}
    for name, src, tgt, T, gate, exact in cases:
        ns, nt, gate2 = len(src), len(tgt), gate * gate
        C2 = planar_cov(rng, nt)
        Tq = [[F_(v) for v in row] for row in T[:3]]
        corr, corr2, und = np.zeros(ns, np.int32), np.zeros(ns, np.int32), np.zeros(ns, bool)
        for i in range(ns):
            p = [F_(v) for v in src[i]]
            q = [Tq[r][0] * p[0] + Tq[r][1] * p[1] + Tq[r][2] * p[2] + Tq[r][3] for r in range(3)]     # real arithmetic on the float entries
            top = exact_nearest(tgt, q, 1)
            d1 = float(top[0][0])
            # the float transform is off by u_q = 3 2^-24 (|T| |p| + |t|) per component; it moves a distance by 2 sqrt(d) |u_q|
            u_q = 0.0 if exact else np.linalg.norm(3 * 2.0 ** -24 * (np.abs(T[:3, :3].astype(np.float64)) @ np.abs(src[i].astype(np.float64)) + np.abs(T[:3, 3])))
            band = lambda d: 0.0 if exact else BAND_D * d + 2 * np.sqrt(d) * u_q
            kept = gate == 0 or top[0][0] < F_(gate2)               # corr = -1 unless d < gate^2
            corr[i] = corr2[i] = top[0][1] if kept else -1
            if kept and not exact and len(top) > 1 and float(top[1][0] - top[0][0]) < 2 * band(float(top[1][0])):
                und[i], corr2[i] = True, top[1][1]                 # (exact arithmetic: a tie goes to the lower index, decided)
            if gate > 0 and not exact and abs(d1 - gate2) < band(d1):
                und[i], corr2[i] = True, (-1 if kept else top[0][1])
        assert und.mean() <= 0.01, (name, und.mean())
        # C1: even points aligned with their target's covariance under R, odd ones at a random orientation
        R = T[:3, :3].astype(np.float64)
        C1 = planar_cov(rng, ns)
        for i in range(0, ns, 2):
            C1[i] = R.T @ C2[max(corr[i], 0)] @ R
        M = np.zeros((ns, 9))
        Rm = mp.matrix([[M_(v) for v in row] for row in R])
        for i in np.flatnonzero(corr >= 0):
            A = Rm * mp.matrix([[M_(v) for v in row] for row in C1[i]]) * Rm.T + mp.matrix([[M_(v) for v in row] for row in C2[corr[i]]])
            Mi = mp.inverse(A)
            M[i] = [float(Mi[a, b]) for a in range(3) for b in range(3)]
        for k, v in (("src", src), ("tgt", tgt), ("C1", C1.reshape(-1, 9)), ("C2", C2.reshape(-1, 9)), ("T", T.reshape(1, 16)), ("gate2", [gate2]),
                     ("corr", corr), ("corr2", corr2), ("M", M), ("und", und), ("ns", [ns]), ("nt", [nt])):
            out[k].append(np.asarray(v))
    k7 = cases.index(next(c for c in cases if c[0] == "c_gate_lattice"))
    lc = out["corr"][k7]
    assert (lc[:27] == -1).all() and (lc[27:54] >= 0).all() and (lc[54:] == -1).all() and not out["und"][k7].any()   # d == gate^2 is rejected
    sc = out["corr"][k7 - 1]
    assert ((sc >= 0) == (np.arange(64) % 2 == 0)).all()
    res = {"co_" + k: np.concatenate(v) for k, v in out.items()}
    res["co_names"] = np.array([c[0] for c in cases])
    return res


def write(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(a), allow_pickle=False)


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 20261019
    rng = np.random.default_rng(seed)
    out = dict(seed=np.int64(seed))
    out.update(make_eval(rng))
    qf = quad_families(rng)
    items = [(n, it) for n in qf for it in qf[n]]
    ex = [quad_exact(*it) for _, it in items]
    out.update(q_names=np.array(list(qf)), q_fam=np.array([list(qf).index(n) for n, _ in items], np.int16), q_abc=np.array([it for _, it in items], np.float64),
               q_count=np.array([e[0] for e in ex], np.int32), q_roots=np.array([[float(e[1]), float(e[2])] for e in ex]))
    fi = interp_families(rng)
    items = [(n, it) for n in fi for it in fi[n]]
    ex = [interp_exact(it) for _, it in items]
    out.update(i_names=np.array(list(fi)), i_fam=np.array([list(fi).index(n) for n, _ in items], np.int16), i_items=np.array([it for _, it in items], np.float64),
               i_alpha=np.array([e[0] for e in ex]), i_other=np.array([e[1] for e in ex]), i_undecidable=np.array([e[2] for e in ex]),
               i_z=np.array([e[3] for e in ex]), i_d2=np.array([e[4] for e in ex]), i_interior=np.array([e[5] for e in ex]), i_cmax=np.array([e[6] for e in ex]))
    for k, n in enumerate(fi):                                     # the families are what their names say, and the cap on ties
        sel = out["i_fam"] == k
        # i_flat is exempt from the cap: a constant function has EVERY candidate tied (the nonzero constants are undecidable by
        # construction, either end is accepted; the zero constant has a zero band and must return the lower end)
        assert out["i_undecidable"][sel].mean() <= 0.01 or n == "i_flat", (n, out["i_undecidable"][sel].mean())
        ends = out["i_items"][sel][:, 6:8]
        al = out["i_alpha"][sel]
        at_lo, at_hi = np.isclose(al, ends[:, 0], rtol=1e-13, atol=0), np.isclose(al, ends[:, 1], rtol=1e-13, atol=0)
        if n in ("i_lower_end", "i_no_stationary", "i_quad_neg", "i_quad_pos_out"):
            assert (at_lo | at_hi).all() and not out["i_interior"][sel].any(), n
        if n == "i_lower_end":
            assert at_lo.all()
        if n == "i_upper_end":
            assert at_hi.all()
        if n in ("i_root1", "i_root2", "i_quad_pos_in", "i_reversed", "i_magnitudes"):
            assert out["i_interior"][sel].all(), n
    assert (out["i_items"][out["i_fam"] == list(fi).index("i_reversed")][:, 0] > out["i_items"][out["i_fam"] == list(fi).index("i_reversed")][:, 3]).all()
    xs = state_cases(rng)
    assert (np.abs(xs[:, 4]) <= 1.5).all()
    out.update(s_x=xs, s_R=np.array([state_exact(x) for x in xs]))
    out.update(round_problems(rng))
    out.update(make_neighbours(rng))
    out.update(make_cov(rng))
    out.update(make_corr(rng))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gicp_kat.npz")
    write(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
