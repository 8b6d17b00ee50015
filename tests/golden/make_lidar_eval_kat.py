"""Known answers for the lidar factor evaluation (line and plane residual rows, their Jacobians, Huber, H / g / cost of a
one-factor problem), computed from the factor's DEFINITION at 80 digits (mpmath), never from the project's formulas:

    R_wb = exp([phi]x) by the exact Rodrigues formula;  P = R_wb (R_bl p + t_bl) + t,  T_bl the 4x4 of doubles given
    line   r = ka (1 - 0.9 ld / |P|^1/2) ld,   ld = |(P - a) x (P - b)| / |a - b|
    plane  r = S (1 - 0.9 |d| / |P|^1/2) d,    d = P - proj,  rows of S: ka w, kb v2, kb v3 with the deterministic basis rule
           (h = the axis of the smallest |w_i|, first on ties; v2 = w x h / |w x h|; v3 = w x v2) on the float omega
    J      central differences of r in x = [t, phi] with step 1e-24 at 80 digits: no left-Jacobian formula anywhere
    Huber  Ceres': rho = s, rho' = 1 for s <= delta^2, else rho = 2 delta sqrt(s) - delta^2, rho' = delta / sqrt(s);  s = sum r^2
    H = rho' J'J (upper triangle, 21), g = rho' J'r, cost = rho / 2;  a record with !(|error| > 1e-5) contributes nothing
    a point exactly on its line: zero residual and zero rows (the project's convention: ld = |.| has no derivative there).
    A point exactly on its plane has a zero residual and the row it has by the definition: |d| d is differentiable at d = 0,
    de/dP = I there, so the row is S dP/dx and H is not zero; g and cost are.

Every value is rounded to double once.  Data only: tests/golden/lidar_eval_kat.npz.

    python tests/golden/make_lidar_eval_kat.py [seed [path]]

`families` names the families, `fam` holds every item's family.  `margin` is the exact s - delta^2 and `band` the width, in
units of s (tests/lidar_eval_checks.py), inside which the Huber branch of an item is undecidable; the generator asserts that at
most 1 % of the Huber families are.
"""
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lidar_eval_checks as K  # noqa: E402  (the units of s, for the band check alone)

mp.mp.dps = 80
STEP = mp.mpf(10) ** -24
LIDAR_M = mp.mpf(1.5e-3)
HUBER = 0.1 / 1.5e-3
W_TAN = 3e-4
BAND = 64.0
THETAS = [(s, float(s)) for s in ("0", "1e-12", "0.99e-10", "1.01e-10", "1e-9", "1.2e-8", "1e-7", "1e-6", "1e-5", "1e-4", "1e-3", "1e-2",
                                  "0.1", "1", "3")] + \
         [("pi-1e-6", float(mp.pi - 1e-6)), ("pi+1e-3", float(mp.pi + 1e-3)), ("2pi-1e-3", float(2 * mp.pi - 1e-3)), ("7", 7.0)]


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def rodrigues(phi):
    th = np.linalg.norm(phi)
    Kx = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    if th == 0:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx


def extrinsics():
    T = np.tile(np.eye(4), (3, 1, 1))
    T[1, :3, :3], T[1, :3, 3] = rodrigues(np.array([0.01, -0.02, 0.015])), [0.05, -0.02, 0.1]
    T[2, :3, :3], T[2, :3, 3] = rodrigues(2.0 * np.array([2.0, -1.0, 2.0]) / 3.0), [0.3, -0.5, 0.8]   # 115 degrees
    return T


T_BL = extrinsics()


# ---------------------------------------------------------------------------------------------------------------------------
# the exact factor
def mpv(a):
    return [mp.mpf(float(v)) for v in a]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def norm(a):
    return mp.sqrt(dot(a, a))


def world_point(x, T, p):
    phi = x[3:6]
    th2 = dot(phi, phi)
    pb = [dot(T[r][:3], p) + T[r][3] for r in range(3)]
    if th2 == 0:
        Rp = pb
    else:
        th = mp.sqrt(th2)
        A, B = mp.sin(th) / th, (1 - mp.cos(th)) / th2
        k1 = cross(phi, pb)
        k2 = cross(phi, k1)
        Rp = [pb[i] + A * k1[i] + B * k2[i] for i in range(3)]
    return [Rp[i] + x[i] for i in range(3)]


def basis(w):
    """the deterministic tangent basis; the comparisons are exact on the floats"""
    a = [abs(v) for v in w]
    h = [1, 0, 0] if a[0] <= a[1] and a[0] <= a[2] else ([0, 1, 0] if a[1] <= a[2] else [0, 0, 1])
    t = cross(w, [mp.mpf(v) for v in h])
    n = norm(t)
    v2 = [v / n for v in t]
    return v2, cross(w, v2)


def rows_exact(kind, x, T, rec, w_tan):
    """-> (rows[3], dist, P)"""
    P = world_point(x, T, rec[0:3])
    ka, kb = 1 / LIDAR_M, mp.mpf(w_tan) / LIDAR_M
    sq = mp.sqrt(norm(P))
    if kind == 0:
        a, b = rec[3:6], rec[6:9]
        ld = norm(cross([P[i] - a[i] for i in range(3)], [P[i] - b[i] for i in range(3)])) / norm([a[i] - b[i] for i in range(3)])
        return [ka * (1 - mp.mpf("0.9") * ld / sq) * ld, mp.mpf(0), mp.mpf(0)], ld, P
    d = [P[i] - rec[3 + i] for i in range(3)]
    nd = norm(d)
    e = [(1 - mp.mpf("0.9") * nd / sq) * v for v in d]
    w = rec[6:9]
    if w_tan == 0:
        return [ka * dot(w, e), mp.mpf(0), mp.mpf(0)], nd, P
    v2, v3 = basis(w)
    return [ka * dot(w, e), kb * dot(v2, e), kb * dot(v3, e)], nd, P


def exact_item(kind, x, tbl, rec, w_tan, delta):
    T = [mpv(row) for row in T_BL[tbl]]
    xm, rm = mpv(x), mpv(rec[:9])
    r, dist, P = rows_exact(kind, xm, T, rm, w_tan)
    zero = kind == 0 and dist == 0
    J = [[mp.mpf(0)] * 6 for _ in range(3)]
    if zero:
        r = [mp.mpf(0)] * 3
    else:
        for c in range(6):
            xp, xn = list(xm), list(xm)
            xp[c] += STEP
            xn[c] -= STEP
            rp, rn = rows_exact(kind, xp, T, rm, w_tan)[0], rows_exact(kind, xn, T, rm, w_tan)[0]
            for q in range(3):
                J[q][c] = (rp[q] - rn[q]) / (2 * STEP)
    s = sum(v * v for v in r)
    d = mp.mpf(float(delta))
    if delta > 0 and s > d * d:
        rho0, rho1 = 2 * d * mp.sqrt(s) - d * d, d / mp.sqrt(s)
    else:
        rho0, rho1 = s, mp.mpf(1)
    err = rec[9]
    excluded = not (abs(err) > 1e-5)
    k = 0 if excluded else 1
    H = [k * rho1 * sum(J[q][a] * J[q][b] for q in range(3)) for a in range(6) for b in range(a, 6)]
    g = [k * rho1 * sum(J[q][a] * r[q] for q in range(3)) for a in range(6)]
    fl = lambda v: [float(t) for t in v]
    return dict(r=fl(r), J=[fl(row) for row in J], s=float(s), rho0=float(rho0), rho1=float(rho1), H=fl(H), g=fl(g),
                cost=float(k * rho0 / 2), margin=float(s - d * d) if delta > 0 else np.nan, dist=float(dist), P=fl(P),
                excluded=excluded, zero=bool(zero))


# ---------------------------------------------------------------------------------------------------------------------------
# items: (kind, x, tbl, rec, w_tan, delta).  The float fields of a record (point, line ends, omega) are floats.
def world64(x, tbl, p):
    T = T_BL[tbl]
    return rodrigues(x[3:]) @ (T[:3, :3] @ p + T[:3, 3]) + x[:3]


def lidar_point(rng, lo=0.5, hi=200.0):
    return f32(unit(rng) * 10.0 ** rng.uniform(np.log10(lo), np.log10(hi)))


def line_item(rng, x, tbl, p, off, seg=0.2, err=0.05, delta=HUBER, keep_pose=False):
    """a line of length seg with float ends near the point, and the translation moved so that the point lies off from it
    (keep_pose: the line is laid off from the point instead, to the rounding of its float ends)"""
    x = np.array(x, float)
    P = world64(x, tbl, p)
    u = unit(rng)
    if keep_pose:
        n = np.cross(u, unit(rng))
        c = P + off * n / np.linalg.norm(n) + rng.uniform(-0.3, 0.3) * seg * u
        return (0, x, tbl, np.concatenate([p, f32(c + 0.5 * seg * u), f32(c - 0.5 * seg * u), [err]]), 0.0, delta)
    c = P + rng.uniform(-0.3, 0.3) * seg * u
    a, b = f32(c + 0.5 * seg * u), f32(c - 0.5 * seg * u)
    u = (a - b) / np.linalg.norm(a - b)
    foot = a + ((P - a) @ u) * u
    n = np.cross(u, unit(rng))
    x[:3] += foot + off * n / np.linalg.norm(n) - P
    return (0, x, tbl, np.concatenate([p, a, b, [err]]), 0.0, delta)


def plane_item(rng, x, tbl, p, off, w_tan, err=0.05, delta=HUBER, omega=None, slant=None):
    """proj = P - off (omega + slant tangent): the tangential rows see a residual where slant != 0"""
    x = np.array(x, float)
    P = world64(x, tbl, p)
    w = f32(unit(rng)) if omega is None else f32(omega)
    tg = np.cross(w, unit(rng))
    sl = (rng.uniform(0, 0.5) if rng.random() < 0.5 else 0.0) if slant is None else slant
    proj = P - off * (w + sl * tg)
    return (1, x, tbl, np.concatenate([p, proj, w, [err]]), w_tan, delta)


def pose(rng, theta, tmax):
    return np.concatenate([rng.uniform(-tmax, tmax, 3), theta * unit(rng)])


def s_of(item):
    """s = sum r^2 in doubles: steers the Huber families only, the stored values are the exact ones"""
    kind, x, tbl, rec, w_tan, _ = item
    P = world64(x, tbl, rec[:3])
    sq = np.sqrt(np.linalg.norm(P))
    if kind == 0:
        a, b = rec[3:6], rec[6:9]
        ld = np.linalg.norm(np.cross(P - a, P - b)) / np.linalg.norm(a - b)
        return (float(1 / LIDAR_M) * (1 - 0.9 * ld / sq) * ld) ** 2
    d = P - rec[3:6]
    e = (1 - 0.9 * np.linalg.norm(d) / sq) * d
    w = rec[6:9]
    s = (float(1 / LIDAR_M) * (w @ e)) ** 2
    if w_tan:
        v2, v3 = basis(mpv(w))
        s += (w_tan / 1.5e-3) ** 2 * ((np.array(v2, float) @ e) ** 2 + (np.array(v3, float) @ e) ** 2)
    return s


def tuned(make, target, lo, hi):
    """bisect the offset to a crossing of s(make(offset)) with target inside [lo, hi]"""
    assert s_of(make(lo)) < target < s_of(make(hi)), (s_of(make(lo)), target, s_of(make(hi)))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if s_of(make(mid)) < target:
            lo = mid
        else:
            hi = mid
    return make(hi)


def families(seed):
    fam = {}
    # ---- rotation magnitude: the same 18 geometries (by seed) at every theta; three T_bl; lines, planes with and without the
    #      tangential rows
    for name, th in THETAS:
        it = []
        for k in range(18):
            rng = np.random.default_rng([seed, 1, k])
            tbl = k % 3
            x = pose(rng, th, 500.0)
            p = lidar_point(rng)
            off = 10.0 ** rng.uniform(-3, -0.5)
            it.append(line_item(rng, x, tbl, p, off))
            it.append(plane_item(rng, x, tbl, p, off, W_TAN if k % 2 else 0.0))
        fam["theta_" + name] = it
    rng = np.random.default_rng([seed, 2])
    gen = lambda: (pose(rng, 10.0 ** rng.uniform(-3, 0), 50.0), int(rng.integers(0, 3)), lidar_point(rng))
    # ---- line geometry
    fam["line_generic"] = [line_item(rng, *gen(), 10.0 ** rng.uniform(-3, -0.5)) for _ in range(60)]
    for off in ("1e-3", "1e-6", "1e-9"):
        fam["line_near_" + off] = [line_item(rng, *gen(), float(off)) for _ in range(40)]
    fam["line_on"] = on_line_items(rng)
    for seg in ("0.2", "1e-3", "10"):
        fam["line_seg_" + seg] = [line_item(rng, *gen(), 10.0 ** rng.uniform(-3, -0.5), seg=float(seg)) for _ in range(16)]
    it = []
    for k in range(24):                                   # |P| from 1 m down to 1e-2 m: the weight goes negative
        x = pose(rng, 10.0 ** rng.uniform(-3, 0), 0.0)
        p = f32(unit(rng) * 10.0 ** (-2 + 2 * (k // 3) / 7))
        it.append(line_item(rng, x, 0, p, [0.02, 0.08, 0.3][k % 3], keep_pose=True))
    fam["line_small_range"] = it
    # ---- plane geometry
    wt = lambda k: W_TAN if k % 2 else 0.0
    fam["plane_generic"] = [plane_item(rng, *gen(), 10.0 ** rng.uniform(-3, -0.5), wt(k)) for k in range(60)]
    for off in ("1e-3", "1e-6", "1e-9"):
        fam["plane_near_" + off] = [plane_item(rng, *gen(), float(off), wt(k)) for k in range(40)]
    fam["plane_on"] = on_plane_items(rng)
    ax = []
    for k in range(24):
        w = np.zeros(3)
        w[k % 3] = 1.0 if k % 2 else -1.0
        ax.append(plane_item(rng, *gen(), 10.0 ** rng.uniform(-3, -0.5), wt(k // 6), omega=w, slant=0.3))
    fam["plane_axis"] = ax
    ties = []
    pat = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (2, 1, 1), (1, 2, 2), (2, 1, 2), (2, 2, 1), (1, -1, 2), (-2, 1, -1), (3, 2, 1), (2, 3, 1),
           (3, 1, 2), (1, 3, 2), (2, 1, 3), (1, 2, 3), (0, 1, 1), (1, 0, 1), (1, 1, 0)]   # every order and every tie of |w0| |w1| |w2|
    for k, w in enumerate(pat + pat):
        w = np.array(w, float) / np.linalg.norm(w)
        w = f32(w)                                                                       # (equal integers give equal floats)
        ties.append(plane_item(rng, *gen(), 10.0 ** rng.uniform(-3, -0.5), W_TAN if k < len(pat) or k % 3 else 0.0, omega=w, slant=0.3))
    fam["plane_basis_ties"] = ties
    it = []
    for k in range(12):
        x = pose(rng, 10.0 ** rng.uniform(-3, 0), 0.0)
        p = f32(unit(rng) * 10.0 ** (-2 + 2 * (k // 3) / 3))
        it.append(plane_item(rng, x, 0, p, [0.02, 0.08, 0.3][k % 3], wt(k)))
    fam["plane_small_range"] = it
    # ---- Huber: delta off; s against delta^2
    fam["huber_off"] = [line_item(rng, *gen(), 10.0 ** rng.uniform(-2, 0.5), delta=0.0) for _ in range(10)] + \
                       [plane_item(rng, *gen(), 10.0 ** rng.uniform(-2, 0.5), wt(k), delta=0.0) for k in range(10)]
    fam["huber_far_below"] = [line_item(rng, *gen(), 10.0 ** rng.uniform(-6, -3)) for _ in range(12)] + \
                             [plane_item(rng, *gen(), 10.0 ** rng.uniform(-6, -3), wt(k)) for k in range(12)]
    d2 = HUBER * HUBER

    def steered(target, lo, hi, k):
        while True:                                        # |P| >= 16 m: s rises with the offset up to 2.2 m and beyond 4.5 sqrt|P|
            x, tbl, p = gen()
            if np.linalg.norm(world64(x, tbl, p)) >= 16.0 and np.linalg.norm(p) <= 120.0:
                break
        st = rng.bit_generator.state
        if k % 2 == 0:
            def make(off):
                rng.bit_generator.state = st
                return line_item(rng, x, tbl, p, off)
        else:
            def make(off):
                rng.bit_generator.state = st
                return plane_item(rng, x, tbl, p, off, wt(k // 2), slant=0.0 if k % 4 == 1 else 0.2)
        return tuned(make, target, lo, hi)
    for side, sg in (("below", -1.0), ("above", 1.0)):
        fam["huber_near_" + side] = [steered(d2 * (1 + sg * m), 0.01, 1.5, k) for k, m in
                                     enumerate([1e-3] * 12 + [1e-5] * 12 + [1e-7] * 12 + [1e-8] * 12 + [1e-9] * 12)]
    fam["huber_10x"] = [steered(10 * d2, 0.01, 2.0, k) for k in range(24)]
    fam["huber_1e6x"] = [steered(1e6 * d2, 5.0, 3000.0, k) for k in range(24)]
    # ---- the error gate: 1e-5 (out), the next double (in), -1e-5 (out), 0 (out), NaN (out)
    gate = []
    for err in (1e-5, np.nextafter(1e-5, 1.0), -1e-5, 0.0, np.nan):
        for k in range(4):
            a = gen()
            gate.append(line_item(rng, *a, 0.02, err=err))
            gate.append(plane_item(rng, *a, 0.02, wt(k), err=err))
    fam["gate"] = gate
    # ---- one pose, 130 lines and 130 planes: the lists of the reduction test (their exact records add up to the exact H, g, cost)
    x = np.concatenate([[3.0, -2.0, 1.0], 1e-6 * unit(rng)])
    fam["one_pose"] = [line_item(rng, x, 1, lidar_point(rng, hi=80.0), 10.0 ** rng.uniform(-3, -0.5), keep_pose=True) for _ in range(130)] + \
                      [plane_item(rng, x, 1, lidar_point(rng, hi=80.0), 10.0 ** rng.uniform(-3, -0.5), 0.0) for _ in range(130)]
    return fam


def on_line_items(rng):
    """the point exactly on its line, and every operation on the way exact: identity extrinsic, no rotation, coordinates that are
    small multiples of 1/8"""
    out = []
    for k in range(12):
        g = lambda: rng.integers(-40, 41, 3) / 8.0
        p, t, h = g(), g(), g()
        h[h == 0] = 0.125
        P = p + t
        a, b = (P + h, P - h) if k % 3 == 0 else ((P, P + h) if k % 3 == 1 else (P + h, P + 3 * h))
        out.append((0, np.concatenate([t, np.zeros(3)]), 0, np.concatenate([p, a, b, [0.05]]), 0.0, HUBER if k % 2 else 0.0))
    return out


def on_plane_items(rng):
    out = []
    for k in range(12):
        g = lambda: rng.integers(-40, 41, 3) / 8.0
        p, t = g(), g()
        out.append((1, np.concatenate([t, np.zeros(3)]), 0, np.concatenate([p, p + t, f32(unit(rng)), [0.05]]), W_TAN if k % 2 else 0.0,
                    HUBER if k % 4 < 2 else 0.0))
    return out


def write_npz(path, arrays):
    """an .npz whose bytes depend on the arrays alone (fixed member times)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(a), allow_pickle=False)


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 20261019
    fam = families(seed)
    names = list(fam)
    items = [(i, it) for i, n in enumerate(names) for it in fam[n]]
    ex = [exact_item(*it) for _, it in items]
    out = dict(families=np.array(names), fam=np.array([i for i, _ in items], np.int16), T_bl=T_BL, seed=np.int64(seed), band=np.float64(BAND),
               kind=np.array([it[0] for _, it in items], np.int8), x=np.array([it[1] for _, it in items]),
               tbl=np.array([it[2] for _, it in items], np.int8), rec=np.array([it[3] for _, it in items]),
               w_tan=np.array([it[4] for _, it in items]), delta=np.array([it[5] for _, it in items]))
    for key in ("r", "J", "s", "rho0", "rho1", "H", "g", "cost", "margin", "dist", "P", "excluded", "zero"):
        out[key] = np.array([e[key] for e in ex])
    # the float fields are floats
    line = out["kind"] == 0
    cols = np.where(line[:, None], np.arange(9)[None, :] >= 0, (np.arange(9) < 3) | (np.arange(9) >= 6))
    assert np.array_equal(np.where(cols, f32(out["rec"][:, :9]), out["rec"][:, :9]), out["rec"][:, :9])
    # at most 1 % of the Huber families inside the band
    u = K.units(out)
    hub = np.array([names[i].startswith("huber_") and names[i] != "huber_off" for i in out["fam"]])
    frac = u["undecidable"][hub].mean()
    print("items %d; undecidable in the Huber families: %d of %d; elsewhere %d" % (len(ex), u["undecidable"][hub].sum(), hub.sum(), u["undecidable"][~hub].sum()))
    assert frac <= 0.01, frac
    near = np.array([names[i].startswith("huber_near") for i in out["fam"]])
    rel = out["margin"][near] / HUBER ** 2
    print("near families: |s / delta^2 - 1| from %.3g to %.3g, %d below, %d above" % (np.abs(rel).min(), np.abs(rel).max(), (rel < 0).sum(), (rel > 0).sum()))
    assert out["zero"].sum() == 12 and (out["dist"] == 0).sum() == 24 and out["excluded"].sum() == 32
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "lidar_eval_kat.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes;", {n: len(fam[n]) for n in names})


if __name__ == "__main__":
    main()
