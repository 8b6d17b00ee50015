"""Shared by tests/test_lidar_eval.py (the oracle, CPU) and tests/test_gpu_lidar_eval.py (the device): worst ratios of an
implementation's single-factor lidar evaluation (residual rows, Jacobians, H = rho' J'J, g = rho' J'r, cost) against the exact
references of tests/golden/lidar_eval_kat.npz, and its gate / zero / Huber-branch decisions against the exact ones.

A ratio is an error divided by a first-order rounding unit: eps = 2^-52 times the exact magnitudes of the operands the
factor's definition combines (units() below, every term commented).  Nothing in a unit is measured on an implementation, and
no unit contains a negative power of the rotation angle: |J_l| enters as 1 + theta / 2 + theta^2 / 6.  The inherent
conditioning of the definition is in the units -- the cross product's eps |P - a| |P - b| / |a - b|, the direction of a
1e-9 m offset known to u / 1e-9 -- because the reference computes the same expressions in the same precision."""
import os

import numpy as np

EPS = 2.0 ** -52
KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar_eval_kat.npz")
LIDAR_M = 1.5e-3
KA = 1.0 / LIDAR_M
ROW_NAMES = ("c_r", "c_jt", "c_jr")                                  # residual rows, dr/dt, dr/dphi
NEQ_NAMES = ("c_htt", "c_htr", "c_hrr", "c_gt", "c_gr", "c_c")       # blocks of H, halves of g, cost
# index pairs of the 21-entry upper triangle (row-major, a <= b)
TRI = [(a, b) for a in range(6) for b in range(a, 6)]
TT = np.array([a < 3 and b < 3 for a, b in TRI])
RR = np.array([a >= 3 and b >= 3 for a, b in TRI])
TR = ~TT & ~RR

# The oracle's worst ratio over the whole fixture (measured on the CPU, tabulated in tests/test_lidar_eval.py); the bounds
# are 8 x these for the oracle and the device alike.
MEASURED = {"c_r": 0.95, "c_jt": 0.68, "c_jr": 0.62, "c_htt": 0.90, "c_htr": 0.89, "c_hrr": 0.88, "c_gt": 0.76, "c_gr": 0.76, "c_c": 0.95}
BOUNDS = {k: 8 * v for k, v in MEASURED.items()}

# the small-angle condition: worst ratio over theta in [1e-10, 1e-4] at most SMALL_ANGLE_FACTOR x the worst over [1e-2, 1]
SMALL_ANGLE_FACTOR = 4.0
SMALL_ANGLE_NAMES = ("c_jt", "c_jr", "c_htt", "c_htr", "c_hrr")


def load(path=KAT):
    z = np.load(path)
    f = {k: z[k] for k in z.files}
    f["families"] = [str(s) for s in f["families"]]
    f.update(units(f))
    return f


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def units(f):
    """First-order rounding units of every stored quantity, from the exact values of the fixture."""
    with np.errstate(all="ignore"):
        n = len(f["kind"])
        line = f["kind"] == 0
        x, rec = f["x"], f["rec"]
        P = f["P"]
        Rpb = P - x[:, :3]                                   # R_wb (R_bl p + t_bl); the magnitude is all that is used
        nP, nR, nt = _norm(P), _norm(Rpb), _norm(x[:, :3])
        th = _norm(x[:, 3:])
        sP = np.sqrt(nP)
        dist = f["dist"]                                     # ld of a line factor, |d| of a plane factor
        w = np.abs(1.0 - 0.9 * dist / sP)
        # P = R_wb (R_bl p + t_bl) + t: two rotations of the lever, one sum
        u_P = EPS * (2 * nR + nt + nP)
        u_nP = u_P + EPS * nP
        # distance: line -- the two products of every cross-product component, over |a - b|; plane -- P - proj
        a, b = rec[:, 3:6], rec[:, 6:9]
        pa, pb, ab = _norm(P - a), _norm(P - b), _norm(a - b)
        u_dist = np.where(line, u_P + EPS * (2 * pa * pb / ab + 4 * dist), u_P + EPS * dist)
        # weight = 1 - 0.9 dist |P|^-1/2
        u_w = EPS * (1 + 6 * 0.9 * dist / sP) + 0.9 * (u_dist / sP + 0.5 * dist * u_nP / (nP * sP))
        # unit direction of the offset (grad of ld; d / |d|): known to u_dist / dist.  The plane rows meet it only multiplied
        # with dist (d_dir), which stays finite for the point exactly on its plane
        u_dir = u_dist / dist + 4 * EPS
        d_dir = u_dist + 4 * EPS * dist
        # gw = d weight / dP = -0.9 (|P|^-1/2 dir - 1/2 dist |P|^-5/2 P); d_gw = dist x its unit
        gw = 0.9 * (1 / sP + 0.5 * dist / (nP * sP))
        d_gw = 0.9 * (d_dir / sP + dist * (0.5 * u_nP / (nP * sP) + 0.5 * u_dist / (nP * sP) + 1.75 * dist * u_nP / (nP * nP * sP))) + 6 * EPS * gw * dist
        # scale of the rows: ka (line; plane row 0: ka |omega|), kb (tangential rows)
        om = _norm(rec[:, 6:9])
        kb = f["w_tan"] / LIDAR_M
        scale = np.stack([np.where(line, KA, KA * om), np.where(line, 0.0, kb), np.where(line, 0.0, kb * om)], 1)
        basis = np.array([0.0, 4.0, 8.0]) * EPS               # the tangent basis: a cross product, a norm; two cross products
        # r = scale weight dist (line), scale weight row . d (plane)
        u_r = scale * ((w * u_dist + dist * u_w + 4 * EPS * w * dist)[:, None] + basis[None, :] * (w * dist)[:, None])
        # gr = dr / dP: line ka (w gl + ld gw); plane w row + (row . d) gw
        u_gr = scale * (np.where(line, w * u_dir, 0.0) + u_w + d_gw + gw * u_dist + 8 * EPS * (w + dist * gw))[:, None] \
            + scale * basis[None, :] * (w + dist * gw)[:, None]
        # J = gr' [I, -[R p_b]x J_l]; |J_l| <= 1 + theta / 2 + theta^2 / 6
        jl = 1 + 0.5 * th + th * th / 6
        J = f["J"]
        gmag = _norm(J[:, :, :3])
        u_jr = jl[:, None] * (u_gr * nR[:, None] + gmag * (u_P + 6 * EPS * nR)[:, None])
        u_J = np.concatenate([np.repeat(u_gr[:, :, None], 3, 2), np.repeat(u_jr[:, :, None], 3, 2)], 2)
        # s = sum r^2, Ceres' Huber: rho = s, rho' = 1 (s <= delta^2) | rho = 2 delta sqrt s - delta^2, rho' = delta / sqrt s
        r, s, delta, rho1 = np.abs(f["r"]), f["s"], f["delta"], f["rho1"]
        u_s = 2 * (r * u_r).sum(1) + 4 * EPS * s
        above = (delta > 0) & (f["margin"] > 0)
        u_rho1 = np.where(above, rho1 * (0.5 * u_s / s + 3 * EPS), 0.0)
        u_c = 0.5 * np.where(above, delta * u_s / np.sqrt(s) + 2 * EPS * (2 * delta * np.sqrt(s) + delta * delta), u_s)
        aJ = np.abs(J)
        u_H = np.empty((n, 21))
        for k, (p, q) in enumerate(TRI):
            u_H[:, k] = rho1 * (aJ[:, :, p] * u_J[:, :, q] + aJ[:, :, q] * u_J[:, :, p]).sum(1) + (u_rho1 + 4 * EPS * rho1) * (aJ[:, :, p] * aJ[:, :, q]).sum(1)
        u_g = rho1[:, None] * (aJ * u_r[:, :, None] + r[:, :, None] * u_J).sum(1) + (u_rho1 + 4 * EPS * rho1)[:, None] * (aJ * r[:, :, None]).sum(1)
        # Huber branch: undecidable where the exact |s - delta^2| is inside the stored band of units of s
        undecidable = (delta > 0) & (np.abs(f["margin"]) <= f["band"] * (u_s + 2 * EPS * delta * delta))
    return dict(u_r=u_r, u_J=u_J, u_s=u_s, u_H=u_H, u_g=u_g, u_c=u_c, undecidable=undecidable)


def by_family(f, ratio):
    """worst ratio per family; a family without a comparable item is NaN"""
    out = {}
    for i, name in enumerate(f["families"]):
        r = ratio[f["fam"] == i]
        out[name] = float(np.nanmax(r)) if np.isfinite(r).any() else float("nan")
    return out


def _ratio(err, unit, live):
    with np.errstate(all="ignore"):
        q = np.where(unit > 0, np.abs(err) / unit, np.where(err == 0, 0.0, np.inf))
    q = q.reshape(len(q), -1).max(1)
    return np.where(live, q, np.nan)


def row_summary(f, rows):
    """rows(i) -> (r[3], J[3, 6]) of item i (the tangential rows zero where w_tan = 0).  Worst ratio per quantity and family,
    and the zero flags: an item exactly on its line has zero rows, one exactly on its line or plane a zero residual, not small
    ones."""
    n = len(f["kind"])
    r, J = np.zeros((n, 3)), np.zeros((n, 3, 6))
    for i in range(n):
        r[i], J[i] = rows(i)
    live = ~f["zero"]
    ratios = {"c_r": by_family(f, _ratio(r - f["r"], f["u_r"], live)),
              "c_jt": by_family(f, _ratio((J - f["J"])[:, :, :3], f["u_J"][:, :, :3], live)),
              "c_jr": by_family(f, _ratio((J - f["J"])[:, :, 3:], f["u_J"][:, :, 3:], live))}
    flags = {"zero rows": live | ((r == 0).all(1) & (J == 0).all((1, 2))), "zero residual": ~(f["r"] == 0).all(1) | (r == 0).all(1), "finite": np.isfinite(r).all(1) & np.isfinite(J).all((1, 2))}
    return ratios, flags


def summary(f, evaluate):
    """evaluate(items) -> (H21, g6, cost): items is an index array into the fixture, every item evaluated as a problem of
    that ONE factor.  Worst ratio per quantity and family; gate, zero and Huber-branch flags."""
    idx = np.arange(len(f["kind"]))
    H, g, c = evaluate(idx)
    live = ~f["zero"] & ~f["excluded"] & ~f["undecidable"]
    eH, eg, ec = H - f["H"], g - f["g"], c - f["cost"]
    ratios = {"c_htt": _ratio(eH[:, TT], f["u_H"][:, TT], live), "c_htr": _ratio(eH[:, TR], f["u_H"][:, TR], live),
              "c_hrr": _ratio(eH[:, RR], f["u_H"][:, RR], live), "c_gt": _ratio(eg[:, :3], f["u_g"][:, :3], live),
              "c_gr": _ratio(eg[:, 3:], f["u_g"][:, 3:], live), "c_c": _ratio(ec, f["u_c"], live)}
    ratios = {k: by_family(f, v) for k, v in ratios.items()}
    nothing = (H == 0).all(1) & (g == 0).all(1) & (c == 0)
    on = (f["r"] == 0).all(1)                                # exactly on its line or plane: no residual
    with np.errstate(all="ignore"):
        # the branch shows in the cost where the two forms of rho differ by more than the cost's bound reaches:
        # rho_below - rho_above = (sqrt s - delta)^2
        s, d = f["s"], f["delta"]
        other = np.where(f["margin"] > 0, 0.5 * s, d * np.sqrt(s) - 0.5 * d * d)
        told = (d > 0) & live & (np.abs(other - f["cost"]) > 4 * max(BOUNDS["c_c"], 8.0) * f["u_c"])
        branch_ok = ~told | (np.abs(c - f["cost"]) < np.abs(c - other))
    flags = {"gate: an excluded record contributes exactly nothing": ~f["excluded"] | nothing,
             "gate: an included record contributes": f["excluded"] | f["zero"] | ~nothing,
             "a point exactly on its line contributes exact zeros": ~f["zero"] | nothing,
             "a point exactly on its line / plane: g and cost exactly zero": ~on | ((g == 0).all(1) & (c == 0)),
             "huber branch": branch_ok, "finite": np.isfinite(H).all(1) & np.isfinite(g).all(1) & np.isfinite(c)}
    return ratios, flags


def theta_classes(f):
    """family names of the rotation sweep with theta in [1e-10, 1e-4] and in [1e-2, 1]"""
    th = {name: float(np.median(_norm(f["x"][f["fam"] == i, 3:]))) for i, name in enumerate(f["families"]) if name.startswith("theta_")}
    return [k for k, v in th.items() if 1e-10 <= v <= 1e-4], [k for k, v in th.items() if 1e-2 <= v <= 1]


def small_angle_condition(f, ratios):
    """{name: (worst small, worst large)} of the ratios that are Jacobian or H ratios; the condition is small <= 4 x large"""
    small, large = theta_classes(f)
    assert len(small) >= 7 and len(large) == 3, (small, large)
    return {k: (max(v[s] for s in small), max(v[s] for s in large)) for k, v in ratios.items() if k in SMALL_ANGLE_NAMES}


# ---- the checks both suites apply to a summary ------------------------------------------------------------------------------
def report(who, ratios):
    """prints every family's ratio; -> the (quantity, family, ratio) outside the bounds"""
    for name, per_family in ratios.items():
        for fam, r in per_family.items():
            print("%s %s %-20s %s" % (who, name, fam, "%8.3f (bound %.1f)" % (r, BOUNDS[name]) if r == r else "exact zeros expected: flags only"))
    assert all(any(r == r for r in pf.values()) for pf in ratios.values())
    return [(n, f, r) for n, pf in ratios.items() for f, r in pf.items() if r == r and not r <= BOUNDS[n]]


def check_flags(who, flags):
    for name, ok in flags.items():
        assert ok.all(), "%s: %s: wrong on items %s" % (who, name, np.flatnonzero(~ok)[:10])


def check_small_angles(who, kat, ratios):
    cond = small_angle_condition(kat, ratios)
    for name, (small, large) in cond.items():
        print("%s %s small angles %.3g, theta in [1e-2, 1] %.3g" % (who, name, small, large))
    bad = {k: v for k, v in cond.items() if not v[0] <= SMALL_ANGLE_FACTOR * v[1]}
    assert not bad, "%s: the error grows as theta shrinks: %s" % (who, bad)


def check_against_exact(kat, evaluate, who):
    """the shared check of an (H, g, cost) evaluation: flags, the small-angle condition, the bounds"""
    ratios, flags = summary(kat, evaluate)
    bad = report(who, ratios)
    check_flags(who, flags)
    check_small_angles(who, kat, ratios)
    assert not bad, "%s outside the bound: %s" % (who, bad)
    return ratios


def oracle_rows(O, f):
    def rows(i):
        T = f["T_bl"][f["tbl"][i]]
        if f["kind"][i] == 0:
            rr, J = O.line_residual(line_records(f["rec"][i:i + 1]), f["x"][i], T)
            return np.array([rr, 0.0, 0.0]), np.stack([J, np.zeros(6), np.zeros(6)])
        return O.plane_residual(plane_records(f["rec"][i:i + 1]), f["x"][i], T, f["w_tan"][i])
    return rows


def line_records(rec):
    """(n, 10) upload records -> the oracle's structured line factors"""
    import mml_oracle as O
    out = np.zeros(len(rec), O.LINE_DT)
    out["point_ori"], out["p1"], out["p2"], out["error"] = rec[:, :3], rec[:, 3:6], rec[:, 6:9], rec[:, 9]
    return out


def plane_records(rec):
    import mml_oracle as O
    out = np.zeros(len(rec), O.PLANE_DT)
    out["point_ori"], out["point_proj"], out["omega"], out["error"] = rec[:, :3], rec[:, 3:6], rec[:, 6:9], rec[:, 9]
    return out


def oracle_evaluate(O, f):
    def evaluate(idx):
        H, g, c = np.zeros((len(idx), 21)), np.zeros((len(idx), 6)), np.zeros(len(idx))
        none_l, none_p = line_records(np.zeros((0, 10))), plane_records(np.zeros((0, 10)))
        for k, i in enumerate(idx):
            one = f["rec"][i:i + 1]
            lf, pf = (line_records(one), none_p) if f["kind"][i] == 0 else (none_l, plane_records(one))
            Hm, g[k], c[k] = O.linearize(lf, pf, f["x"][i], f["T_bl"][f["tbl"][i]], f["w_tan"][i], f["delta"][i])
            H[k] = [Hm[a, b] for a, b in TRI]
        return H, g, c
    return evaluate
