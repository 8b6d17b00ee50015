"""Shared by tests/test_gicp_kat.py (the oracle, CPU) and tests/test_gpu_gicp_kat.py (the device, through mml_debug_gicp): the
pieces of the GICP against the exact references of tests/golden/gicp_kat.npz (tests/golden/make_gicp_kat.py).

A ratio is an error divided by a first-order rounding unit formed from the definition and the exact magnitudes of its operands;
nothing in a unit is measured on an implementation.  BOUNDS = 8 x MEASURED, the oracle's worst ratios (tabulated in
tests/test_gicp_kat.py), for the oracle and the device alike.  An implementation is a dict of callables:
  neigh(pts) -> ids[n, 20]     cov(pts) -> C[n, 3, 3]     corr(src, tgt, C1, C2, T, gate2) -> (corr[n], M[n, 3, 3])
  eval(src, tgt, corr, maha, xs, gated) -> (f[K], g[K, 6])     corr holds -1 at a hole (only when gated)
  quad(abc) -> (count[n], roots[n, 2])        interp(items) -> alpha[n]        state(xs) -> (T[n, 4, 4] float32, x[n, 6])
  round(src, tgt, corr, maha, T, gate2, max_iterations, transformation_epsilon) -> dict(T, converged, failed, nr, evals, fobj, delta)
"""
import math
import os
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
EPSF = 2.0 ** -24
KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gicp_kat.npz")

# The oracle's worst ratio per quantity over the whole fixture, measured on the CPU (tests/test_gicp_kat.py prints the table)
MEASURED = {"f": 0.021, "g_t": 0.046, "g_r": 0.017, "quad": 1.0, "interp": 0.13, "state_R": 0.47, "state_x": 0.23, "round_f": 0.006, "cov": 0.038, "maha": 1.0}
BOUNDS = {k: 8 * v for k, v in MEASURED.items()}

# ---- objective: lists and states ------------------------------------------------------------------------------------------------
EVAL_N = 1537
EVAL_M = (4, 5, 511, 512, 513, 1024, 1025, 1537)       # either side of the 512-term LDS chunks, the 1024-point tiles, the 256-lane blocks
SEAMS = (255, 256, 257, 511, 512, 513, 767, 768, 1023, 1024, 1025, 1279, 1280, 1535)
# x = (t, roll, pitch, yaw): angle 1e-6 on each axis alone, 1e-3 on all, two states where every entry of the three derivative
# matrices is O(1), theta = +-1.5, the zero state; translations 0, 0.05 and 5 go round
EVAL_STATES = np.array([
    (0, 0, 0, 1e-6, 0, 0), (0.05, -0.05, 0.05, 0, 1e-6, 0), (5, -5, 5, 0, 0, 1e-6), (0.05, 0.05, -0.05, 1e-3, 1e-3, 1e-3),
    (0, 0, 0, 0.3, -0.4, 0.5), (5, 5, -5, -2.5, 1.2, 2.8), (0.05, 0, 5, 0.3, -0.4, 0.5), (0, 0.05, 0, -2.5, 1.2, 2.8),
    (0, 0, 0, 0.7, 1.5, -0.9), (-5, 0.05, 0, -0.7, -1.5, 2.0), (0, 0, 0, 0, 0, 0)], dtype=np.float64)
EVAL_O1 = (4, 5, 6, 7)


def eval_lists():
    """[(n positions, hole positions)]: every m without holes, every m with holes at the first, the last and the seam positions,
    and the longest list with every second entry a hole"""
    out = [(m, np.zeros(0, int)) for m in EVAL_M]
    for m in EVAL_M:
        out.append((m, np.array(sorted({0, m - 1} | {s for s in SEAMS if s < m - 1}))))
    out.append((EVAL_N, np.arange(1, EVAL_N, 2)))
    return out


def load(path=KAT):
    z = np.load(path)
    f = {k: z[k] for k in z.files}
    for k in ("q_names", "i_names", "nn_names", "cv_names", "co_names"):
        f[k] = [str(s) for s in f[k]]
    return f


def rotation(x):
    """Rz Ry Rx in doubles (for magnitudes only)"""
    cx, sx, cy, sy, cz, sz = math.cos(x[3]), math.sin(x[3]), math.cos(x[4]), math.sin(x[4]), math.cos(x[5]), math.sin(x[5])
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def objective_units(p, q, M, R, t):
    """Units of f, of the translation gradient (3) and of a rotation gradient component, for kept points p -> q with matrices M
    under the transformation (R, t).  The evaluated transformation is a float matrix of float-rounded angles:
      u_res = 2^-24 c (|R| |p| + |t| + |q|) per component, c = 12: 4.7 for the three angles rounded to float (pi 2^-25 each, times
      |p|), 3 for an entry of the float product Rz Ry Rx, 3 for the float products and sums of the transform, 1 for the float
      subtraction; the translation rounds to float once (inside c).  |R| |p| (entry-wise) stands for the issue's |R p|: a deliberate
      upper bound, as c = 12 is -- both only scale the ratios that MEASURED is taken from.
      f:   1/m sum 2 |res|' |M| u_res                      (first order of res' M res)   + 2^-52 log2(m) 1/m sum |res|' |M| |res|
      g_t: 2/m sum |M| u_res                               (g_t = 2/m sum M res)         + 2^-52 log2(m) 2/m sum |M| |res|
      g_r: 2/m sum (sum_i (|M| u_res)_i) (sum_j |p_j|)     (g_r = <dR, 2/m sum (M res) p'>, |dR_ij| <= 1) + the same with |res|"""
    m = len(p)
    p, q = p.astype(np.float64), q.astype(np.float64)
    res = p @ R.T + t - q
    u_res = EPSF * 12.0 * (np.abs(p) @ np.abs(R).T + np.abs(t) + np.abs(q))
    aM = np.abs(M)
    Mu = np.einsum("nij,nj->ni", aM, u_res)
    Mr = np.einsum("nij,nj->ni", aM, np.abs(res))
    lg = EPS * max(1.0, math.log2(m))
    u_f = (2 * (np.abs(res) * Mu).sum() + lg * (np.abs(res) * Mr).sum()) / m
    u_gt = (2 * Mu.sum(0) + lg * 2 * Mr.sum(0)) / m
    sp = np.abs(p).sum(1)
    u_gr = (2 * (Mu.sum(1) * sp).sum() + lg * 2 * (Mr.sum(1) * sp).sum()) / m
    return u_f, u_gt, u_gr


def eval_kept(f, li):
    n, holes = eval_lists()[li]
    keep = np.ones(n, bool)
    keep[holes] = False
    idx = np.flatnonzero(keep)
    return n, holes, idx


def eval_units(f):
    lists = eval_lists()
    u_f, u_g = np.zeros((len(lists), len(EVAL_STATES))), np.zeros((len(lists), len(EVAL_STATES), 6))
    for li in range(len(lists)):
        _, _, idx = eval_kept(f, li)
        p, q, M = f["ev_src"][idx], f["ev_tgt"][f["ev_corr"][idx]], f["ev_maha"][idx].reshape(-1, 3, 3)
        for si, x in enumerate(EVAL_STATES):
            a, b, c = objective_units(p, q, M, rotation(x), x[:3])
            u_f[li, si], u_g[li, si, :3], u_g[li, si, 3:] = a, b, c
    return dict(u_f=u_f, u_g=u_g)


def eval_dfdR(f, li, x):
    """df/dR = 2/m sum (M res) p' in doubles (a magnitude for the generator's visibility assertion)"""
    _, _, idx = eval_kept(f, li)
    p, q, M = f["ev_src"][idx].astype(np.float64), f["ev_tgt"][f["ev_corr"][idx]].astype(np.float64), f["ev_maha"][idx].reshape(-1, 3, 3)
    res = p @ rotation(x).T + x[:3] - q
    return 2.0 / len(idx) * np.einsum("ni,nj->ij", np.einsum("nij,nj->ni", M, res), p)


def eval_ratios(f, impl, who):
    """worst ratios of f, g_t, g_r per list; the two variants of a list (a gated call with no hole, an ungated call) where it has none"""
    u = eval_units(f)
    worst = {"f": 0.0, "g_t": 0.0, "g_r": 0.0}
    for li, (n, holes) in enumerate(eval_lists()):
        corr = f["ev_corr"][:n].copy()
        corr[holes] = -1
        for gated in ((True,) if len(holes) else (False, True)):
            fv, gv = impl["eval"](f["ev_src"][:n], f["ev_tgt"], corr, f["ev_maha"][:n], EVAL_STATES, gated)
            assert np.isfinite(fv).all() and np.isfinite(gv).all(), (who, li)
            rf = np.abs(fv - f["ev_f"][li]) / u["u_f"][li]
            rg = np.abs(gv - f["ev_g"][li]) / u["u_g"][li]
            print("%s eval n %4d holes %3d gated %d: f %.3f  g_t %.3f  g_r %.3f   (worst state %d / %d / %d)" % (
                who, n, len(holes), gated, rf.max(), rg[:, :3].max(), rg[:, 3:].max(), rf.argmax(), rg[:, :3].max(1).argmax(), rg[:, 3:].max(1).argmax()))
            worst = {"f": max(worst["f"], rf.max()), "g_t": max(worst["g_t"], rg[:, :3].max()), "g_r": max(worst["g_r"], rg[:, 3:].max())}
    return worst


# ---- solve_quadratic ------------------------------------------------------------------------------------------------------------
def quad_ratios(f, impl, who):
    """count and order exactly; a root in units of 2^-52 |root| (a zero root exactly)"""
    cnt, roots = impl["quad"](f["q_abc"])
    assert np.array_equal(cnt, f["q_count"]), (who, np.flatnonzero(cnt != f["q_count"]))
    worst = {}
    for k, name in enumerate(f["q_names"]):
        sel = np.flatnonzero(f["q_fam"] == k)
        w = 0.0
        for i in sel:
            for j in range(min(f["q_count"][i], 2)):
                want, got = f["q_roots"][i, j], roots[i, j]
                if want == 0:
                    assert got == 0, (who, name, i)
                else:
                    w = max(w, abs(got - want) / (EPS * abs(want)))
            if f["q_count"][i] == 2:
                assert roots[i, 0] <= roots[i, 1], (who, name, i)
        worst[name] = w
        print("%s quadratic %-12s %3d items: worst %.3f" % (who, name, len(sel), w))
    return {"quad": max(worst.values())}


# ---- interpolate ----------------------------------------------------------------------------------------------------------------
def interp_units(f):
    """alpha = a + z h, h = b - a, z the minimiser in the unit interval's coordinate.
      every z:    4 2^-52 |z|  (the roundings of xmin - a, b - a and their quotient)  +  2^-52 (|xmin| + |a|) / |h|  (the cancellation in xmin - a)
      interior z: + 2^-52 (|fp0| + 2 F |z| + 3 F z^2) / |p''(z)|: a root of p' = c1 + 2 c2 z + 3 c3 z^2 moves by the coefficients'
                  perturbation over |p''|; c1 = fp0, and c2, c3 are sums of f0, f1, fp0, fp1 with weights up to 3, 3, 2, 1: F
      alpha:      |h| u_z  +  2^-52 (|a| + |z h|)"""
    it = f["i_items"]
    a, fa, fpa, b, fb, fpb, xmin, xmax = it.T
    h = b - a
    fp0, fp1 = np.abs(fpa * h), np.abs(np.where(np.isfinite(fpb), fpb, 0.0) * h)
    F = 3 * (np.abs(fa) + np.abs(fb)) + 2 * fp0 + fp1
    z = np.abs(f["i_z"])
    end = np.where(np.isclose(f["i_z"] * h + a, xmin, rtol=1e-9, atol=0), xmin, xmax)
    u_z = EPS * (4 * z + (np.abs(end) + np.abs(a)) / np.abs(h))
    with np.errstate(all="ignore"):
        u_z = u_z + np.where(f["i_interior"], EPS * (fp0 + 2 * F * z + 3 * F * z * z) / f["i_d2"], 0.0)
    return np.abs(h) * u_z + EPS * (np.abs(a) + np.abs(z * h))


def interp_ratios(f, impl, who):
    got = impl["interp"](f["i_items"])
    u = interp_units(f)
    assert np.isfinite(got).all()
    r = np.abs(got - f["i_alpha"]) / u
    r2 = np.abs(got - f["i_other"]) / u
    r = np.where(f["i_undecidable"], np.minimum(r, r2), r)          # undecidable: either of the two best candidates
    for k, name in enumerate(f["i_names"]):
        sel = f["i_fam"] == k
        print("%s interpolate %-16s %3d items (%d undecidable): worst %.3f" % (who, name, sel.sum(), f["i_undecidable"][sel].sum(), r[sel].max()))
    return {"interp": r.max()}


# ---- state ----------------------------------------------------------------------------------------------------------------------
def state_ratios(f, impl, who):
    """R against Rz Ry Rx of the float-rounded angles in units of 3 2^-24 (two float products of three terms over entries of at
    most 1, and the float sine / cosine); the translation column exactly the float of x.  The recovered angles against x, modulo
    2 pi, in units of 2^-24 (6 / |cos theta| + |angle|): atan2 of two entries that carry cos theta as a factor and 3 2^-24 of error
    each, asin's slope 1 / cos theta, and the angle's own rounding to float."""
    T, back = impl["state"](f["s_x"])
    x = f["s_x"]
    assert np.array_equal(T[:, :3, 3], x[:, :3].astype(np.float32)) and np.array_equal(back[:, :3], x[:, :3].astype(np.float32).astype(np.float64))
    assert (T[:, 3] == np.array([0, 0, 0, 1], np.float32)).all()
    rR = np.abs(T[:, :3, :3].astype(np.float64) - f["s_R"]) / (3 * EPSF)
    d = back[:, 3:] - x[:, 3:]
    d = np.abs((d + np.pi) % (2 * np.pi) - np.pi)
    rx = d / (EPSF * (6 / np.abs(np.cos(x[:, 4:5])) + np.abs(x[:, 3:])))
    print("%s state: R worst %.3f (item %d), recovered angles worst %.3f (item %d)" % (who, rR.max(), rR.reshape(len(x), -1).max(1).argmax(), rx.max(), rx.max(1).argmax()))
    return {"state_R": rR.max(), "state_x": rx.max()}


# ---- one round ------------------------------------------------------------------------------------------------------------------
def f_exact(src, tgt, corr, maha, T):
    """1/m sum res' M res over the kept correspondences with the FLOAT matrix T, in exact rational arithmetic"""
    Fr = lambda a: [Fraction(float(v)) for v in np.asarray(a).reshape(-1)]
    Tm = Fr(T)
    tot, m = Fraction(0), 0
    for i in np.flatnonzero(corr >= 0):
        p, q, M = Fr(src[i]), Fr(tgt[corr[i]]), Fr(maha[i])
        r = [Tm[4 * k] * p[0] + Tm[4 * k + 1] * p[1] + Tm[4 * k + 2] * p[2] + Tm[4 * k + 3] - q[k] for k in range(3)]
        tot += sum(r[a] * M[3 * a + b] * r[b] for a in range(3) for b in range(3))
        m += 1
    return tot / m


def round_cases(f, O):
    """[(name, src, tgt, corr, maha, T_in, gate2, settings)]: the two problems with the oracle's own covariances and
    correspondence step as inputs, and the 300-point one cut down to 3 and to 4 kept correspondences"""
    out = []
    T0 = np.eye(4, dtype=np.float32)
    for name, settings in (("r300", (10, 1e-6)), ("r513", (500, 1e-3))):
        src, tgt, gate = f[name + "_src"], f[name + "_tgt"], float(f[name + "_gate"])
        corr, maha = O.gicp_correspond(src, tgt, O.gicp_covariances(src), O.gicp_covariances(tgt), T0, gate * gate)
        out.append((name, src, tgt, corr, maha.reshape(-1, 9), T0, gate * gate, settings))
        if name == "r513":
            assert 4 < (corr < 0).sum() < 100
        else:
            for m in (3, 4):
                c = corr.copy()
                c[np.arange(len(c)) % 60 >= 1] = -1
                c[np.flatnonzero(c >= 0)[m:]] = -1
                assert (c >= 0).sum() == m
                out.append(("%s_m%d" % (name, m), src, tgt, c, maha.reshape(-1, 9), T0, 4.0, (1, 1e-6)))
    return out


def round_checks(f, impl, O, who):
    worst = 0.0
    for name, src, tgt, corr, maha, T0, gate2, (max_it, teps) in round_cases(f, O):
        r = impl["round"](src, tgt, corr, maha, T0, gate2, max_it, teps)
        m = int((corr >= 0).sum())
        if m < 4:
            assert r["failed"] == 1 and np.array_equal(r["T"], T0) and r["nr"] == 0 and r["converged"] == 0, (who, name, r)
            continue
        assert r["failed"] == 0 and r["nr"] == 1 and r["evals"] >= 1, (who, name, r)
        Tn = r["T"]
        # the header's rule: delta = largest |T_in - T_out| over 2e-3 (rotation block) or the transformation epsilon (elsewhere)
        ratio = np.full((4, 4), 1.0 / teps)
        ratio[:3, :3] = 1.0 / 2e-3
        delta = (ratio * np.abs(T0.astype(np.float64) - Tn.astype(np.float64))).max()
        assert r["delta"] == delta and r["converged"] == int(1 >= max_it or delta < 1), (who, name, r, delta)
        keep = corr >= 0
        u_f, _, _ = objective_units(src[keep], tgt[corr[keep]], maha[keep].reshape(-1, 3, 3), Tn[:3, :3].astype(np.float64), Tn[:3, 3].astype(np.float64))
        f_new, f_old = f_exact(src, tgt, corr, maha, Tn), f_exact(src, tgt, corr, maha, T0)
        ratio_f = abs(float(Fraction(float(r["fobj"])) - f_new)) / u_f
        print("%s round %-8s m %3d: evals %d delta %.3g converged %d  f %.6g -> %.6g  |fobj - exact f(T)| %.3f units" % (
            who, name, m, r["evals"], r["delta"], r["converged"], float(f_old), float(f_new), ratio_f))
        assert f_new <= f_old, (who, name)
        worst = max(worst, ratio_f)
    return {"round_f": worst}


# ---- neighbours ----------------------------------------------------------------------------------------------------------------
BAND_D = 4 * EPSF                                                  # float rounding of (dx^2 + dy^2) + dz^2, relative to d


def nn_checks(f, impl, who):
    """Discrete: a decidable point's 20 ids are the exact set (the lattice family, whose distances are all exact in float: the exact
    ORDER as well, ties by index); an undecidable one's are a valid set inside the band -- 20 distinct ids, none beyond
    d20 (1 + band), every point closer than d20 (1 - band) among them (doubles resolve the band 1e9 times over)."""
    for k, name in enumerate(f["nn_names"]):
        lo, hi = f["nn_off"][k], f["nn_off"][k + 1]
        pts, want = f["nn_pts"][lo:hi], f["nn_ids"][lo:hi].astype(int)
        got = np.asarray(impl["neigh"](pts)).astype(int)
        und = f["nn_undecidable"][lo:hi]
        assert got.shape == want.shape and (got >= 0).all() and (got < len(pts)).all(), (who, name)
        same_set = (np.sort(got, 1) == np.sort(want, 1)).all(1)
        assert same_set[~und].all(), (who, name, np.flatnonzero(~same_set & ~und)[:5])
        if str(name) == "nn_lattice":
            assert np.array_equal(got, want), (who, name)
        for i in np.flatnonzero(und):
            d = ((pts.astype(np.float64) - pts[i].astype(np.float64)) ** 2).sum(1)
            d20 = f["nn_d20"][lo + i]
            assert len(set(got[i])) == 20 and (d[got[i]] <= d20 * (1 + BAND_D)).all() and set(np.flatnonzero(d < d20 * (1 - BAND_D))) <= set(got[i]), (who, name, i)
        print("%s neighbours %-16s %4d points (%d undecidable): sets equal" % (who, name, len(pts), und.sum()))


# ---- covariance ----------------------------------------------------------------------------------------------------------------
COV_BAND = 0.02                                                    # first-order turn of u0 above which only the spectrum is checked


def cov_first_order(f):
    """PCL forms the second moments from FLOAT products: each is off by 2^-24 |p|^2 at most, the moments by that (plus the double
    sums' 2^-52 terms, 8 of them), which turns u0 by that amount over the gap lambda_1 - lambda_0; u0 u0' moves by twice the turn"""
    maxp2 = (f["cv_pts"].astype(np.float64) ** 2).sum(2).max(1)
    return 2 * (EPSF + 8 * EPS) * maxp2 / f["cv_gap"]


def cov_ratios(f, impl, who):
    """the 20 covariances of a 20-point cloud (one neighbour order per point) against I - (1 - 1e-3) u0 u0' in units of
    cov_first_order + 2^-52; an item whose first-order turn exceeds COV_BAND: the spectrum {1e-3, 1, 1} to 1e-9, symmetric to 4 eps"""
    unit = cov_first_order(f) + EPS
    worst = {}
    for k, name in enumerate(f["cv_names"]):
        w = 0.0
        for i in np.flatnonzero(f["cv_fam"] == k):
            C = np.asarray(impl["cov"](f["cv_pts"][i])).reshape(20, 3, 3)
            assert np.isfinite(C).all()
            if f["cv_spectrum_only"][i]:
                ev = np.linalg.eigvalsh((C + C.transpose(0, 2, 1)) / 2)
                assert np.abs(ev - [1e-3, 1, 1]).max() < 1e-9 and np.abs(C - C.transpose(0, 2, 1)).max() <= 4 * EPS, (who, name, i)
            else:
                w = max(w, np.abs(C - f["cv_C"][i].reshape(3, 3)).max() / unit[i])
        worst[str(name)] = w
        print("%s covariance %-20s worst %.3f  (%d spectrum only)" % (who, name, w, f["cv_spectrum_only"][f["cv_fam"] == k].sum()))
    return {"cov": max(worst.values())}


# ---- correspondence and Mahalanobis --------------------------------------------------------------------------------------------
def corr_ratios(f, impl, who):
    """corr equals the exact one (an undecidable point: either of the two stored candidates); M against the exact inverse in
    units of 2^-52 cond |M| (cond in the 2-norm, |M| the largest entry), zeros where the gate rejects"""
    so = np.concatenate([[0], np.cumsum(f["co_ns"])])
    to = np.concatenate([[0], np.cumsum(f["co_nt"])])
    worst = 0.0
    for k, name in enumerate(f["co_names"]):
        a, b = so[k], so[k + 1]
        tgt, C2 = f["co_tgt"][to[k]:to[k + 1]], f["co_C2"][to[k]:to[k + 1]]
        corr, M = impl["corr"](f["co_src"][a:b], tgt, f["co_C1"][a:b], C2, f["co_T"][k], float(f["co_gate2"][k]))
        M = np.asarray(M).reshape(-1, 9)
        want, alt, und = f["co_corr"][a:b], f["co_corr2"][a:b], f["co_und"][a:b]
        ok = (corr == want) | (und & (corr == alt))
        assert ok.all(), (who, name, np.flatnonzero(~ok)[:5], corr[~ok][:5], want[~ok][:5])
        assert (M[corr < 0] == 0).all(), (who, name)
        sel = np.flatnonzero((corr == want) & (want >= 0))
        Me = f["co_M"][a:b][sel].reshape(-1, 3, 3)
        cond = np.linalg.cond(Me)
        r = np.abs(M[sel].reshape(-1, 3, 3) - Me).max((1, 2)) / (EPS * cond * np.abs(Me).max((1, 2))) if len(sel) else np.zeros(1)
        print("%s correspond %-24s %4d x %4d: %4d rejected, %d undecidable, M worst %.3f" % (who, name, b - a, len(tgt), (corr < 0).sum(), und.sum(), r.max()))
        worst = max(worst, r.max())
    return {"maha": worst}


def oracle_impl(O):
    def ev(src, tgt, corr, maha, xs, gated):
        idx = np.flatnonzero(corr >= 0)
        out = [O.gicp_objective(src, tgt, idx, corr[idx], maha, x) for x in xs]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])
    return dict(neigh=O.gicp_neighbours, cov=O.gicp_covariances, corr=O.gicp_correspond, eval=ev, quad=O.gicp_solve_quadratic, interp=O.gicp_interpolate, state=O.gicp_state,
                round=lambda s, t, c, m, T, g2, mi, te: O.gicp_round(s, t, c, m, T, mi, te))


def check_bounds(who, ratios):
    bad = {k: v for k, v in ratios.items() if not v <= BOUNDS[k]}
    print("%s worst ratios: %s" % (who, {k: "%.3f" % v for k, v in ratios.items()}))
    assert not bad, "%s outside the bound: %s (bounds %s)" % (who, bad, {k: BOUNDS[k] for k in bad})
