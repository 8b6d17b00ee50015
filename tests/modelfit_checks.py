"""Shared by tests/test_modelfit.py (the oracle, CPU) and tests/test_gpu_modelfit.py (the device): worst ratios of an
implementation's model-fit outputs against the exact references of tests/golden/modelfit_kat.npz, in the units of the
bounds of tests/test_modelfit.py's docstring, and its decisions against the exact ones."""
import os

import numpy as np

EPS, EPSF, TINY = 2.0 ** -52, 2.0 ** -23, 2.0 ** -1074
EIG3, QR, LINE, PLANE, OPS64, OPS32 = range(6)
KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "modelfit_kat.npz")

# 4 x the oracle's worst ratio over the fixture (measured on the CPU, see tests/test_modelfit.py)
MEASURED = {"c_e": 10.04, "c_v": 9.43, "c_o": 10.07, "c_q": 2.30, "c_r": 0.365, "c_f": 1.25, "c_p": 0.57, "c_c": 1.20, "c_l": 0.378,
            "c_d": 0.83, "c_t": 1.35}
BOUNDS = {k: 4 * v for k, v in MEASURED.items()}


def load():
    z = np.load(KAT)
    f = {k: z[k] for k in z.files}
    f["qr_in"] = f["qr_in"].astype(np.float64)
    f["plane_in"] = np.concatenate([f["qr_in"].astype(np.float32), f["plane_sel"]], 1)
    return f


def _sym(m):
    A = np.empty((len(m), 3, 3))
    A[:, 0, 0], A[:, 1, 0], A[:, 1, 1], A[:, 2, 0], A[:, 2, 1], A[:, 2, 2] = m.T
    A[:, 0, 1], A[:, 0, 2], A[:, 1, 2] = A[:, 1, 0], A[:, 2, 0], A[:, 2, 1]
    return A


def by_family(names, fam, r):
    """worst ratio per family; a family without a single comparable item (every ratio NaN: no exact value, or all of its
    items undecidable) is reported as NaN, not left out"""
    return {str(n): (float(np.nanmax(r[fam == i])) if np.isfinite(r[fam == i]).any() else float("nan")) for i, n in enumerate(names)}


def eig3_ratios(f, out):
    """out: (n, 12) ev[3], v0, v1, v2.  -> eigenvalue, residual and orthonormality ratios per item, order flag"""
    with np.errstate(all="ignore"):
        A = _sym(f["eig3_in"])
        ev, V = out[:, :3], out[:, 3:].reshape(-1, 3, 3).transpose(0, 2, 1)  # V[:, :, k] = eigenvector k
        den = EPS * np.abs(f["eig3_in"]).max(1) + TINY
        r_e = np.abs(ev - f["eig3_ev"]).max(1) / den
        r_v = np.linalg.norm(A @ V - V * ev[:, None, :], axis=1).max(1) / den
        r_o = np.linalg.norm(V.transpose(0, 2, 1) @ V - np.eye(3), axis=(1, 2)) / EPS
        ordered = (ev[:, 0] <= ev[:, 1]) & (ev[:, 1] <= ev[:, 2])
    return r_e, r_v, r_o, ordered


def qr_ratios(f, out):
    """out: (n, 4) X[3], rank.  Full exact rank away from the threshold: ||X - Xx|| / (eps kappa^2 ||Xx||); every item with an
    exact value: | ||A X + 1|| - exact | / (eps sqrt5 (1 + ||A|| ||X||)); rank against the exact rank where decidable."""
    with np.errstate(all="ignore"):
        A = f["qr_in"].reshape(-1, 5, 3)
        X, rank = out[:, :3], out[:, 3]
        decid = f["qr_rank_margin"] > np.log2(f["bands"][3])
        full = decid & (f["qr_rank"] == 3) & np.isfinite(f["qr_x"]).all(1)
        r_q = np.where(full, np.linalg.norm(X - f["qr_x"], axis=1) / (EPS * f["qr_kappa"] ** 2 * np.linalg.norm(f["qr_x"], axis=1)), np.nan)
        res = np.linalg.norm(np.einsum("nrc,nc->nr", A, X) + 1, axis=1)
        have = decid & np.isfinite(f["qr_resid"])
        den = EPS * np.sqrt(5) * (1 + np.linalg.norm(A, axis=(1, 2)) * np.linalg.norm(X, axis=1)) * np.where(full, f["qr_kappa"], 1.0)
        r_r = np.where(have, np.abs(res - f["qr_resid"]) / den, np.nan)
        rank_ok = ~decid | (rank == f["qr_rank"])
    return r_q, r_r, rank_ok, decid


def plane_ratios(f, out, b_q):
    """out: (n, 11) accepted, X[3], pa pb pc pd, proj[3].  b_q: the QR bound (the share of the double error in the float tail)."""
    with np.errstate(all="ignore"):
        acc, co, proj = out[:, 0] > 0, out[:, 4:8], out[:, 8:11]
        cx = f["plane_coef"]
        decid = ~f["plane_undecidable"]
        unit = EPSF + b_q * EPS * f["qr_kappa"] ** 2
        d = np.abs(co - cx)
        d[:, 3] /= np.abs(cx[:, 3])
        r_f = np.where(decid, d.max(1) / unit, np.nan)
        want = f["plane_margin"] > 0
        dec_ok = ~decid | (acc == want)
        sel = f["plane_sel"].astype(np.float64)
        r_p = np.where(decid & want & acc, np.abs(proj - f["plane_proj"]).max(1) / (unit * (np.abs(sel).max(1) + np.abs(cx[:, 3]) + 1)), np.nan)
    return r_f, r_p, dec_ok, decid


def line_ratios(f, out):
    """out: (n, 13) accepted, centroid[3], ev[3], p1[3], p2[3]"""
    with np.errstate(all="ignore"):
        acc, cen, ev, p1, p2 = out[:, 0] > 0, out[:, 1:4], out[:, 4:7], out[:, 7:10], out[:, 10:13]
        pmax = np.abs(f["line_in"]).max(1).astype(np.float64)
        s = f["line_scale"]
        unit = EPSF * (s + pmax * np.sqrt(s)) + (EPSF * pmax) ** 2 + TINY  # float covariance about a float centroid
        r_c = np.abs(cen - f["line_cen"]).max(1) / (EPSF * pmax + TINY)
        r_l = np.abs(ev - f["line_ev"]).max(1) / unit
        decid = ~f["line_undecidable"]
        want = f["line_ev"][:, 2] > 3 * f["line_ev"][:, 1]
        dec_ok = ~decid | (acc == want)
        both = decid & want & acc
        d = p1 - p2
        sin = np.linalg.norm(np.cross(d, f["line_dir"]), axis=1) / np.linalg.norm(d, axis=1)
        gap = f["line_ev"][:, 2] - f["line_ev"][:, 1]
        r_d = np.where(both, sin / (unit / gap + EPSF * pmax / 0.2 + EPSF), np.nan)
        # the tripod: centre = centroid, length 0.2, to the float rounding of its ends
        mid = np.abs((p1 + p2) / 2 - cen).max(1)
        ln = np.abs(np.linalg.norm(d, axis=1) - 0.2)
        r_t = np.where(both, np.maximum(mid, ln) / (EPSF * (pmax + 0.2)), np.nan)
    return r_c, r_l, r_d, r_t, dec_ok, decid


def summary(f, fit):
    """fit(op, items) -> outputs.  Worst ratio per quantity and family, and the decision / order failures."""
    o_e, o_q = fit(EIG3, f["eig3_in"]), fit(QR, f["qr_in"])
    o_l, o_p = fit(LINE, f["line_in"]), fit(PLANE, f["plane_in"])
    r_e, r_v, r_o, ordered = eig3_ratios(f, o_e)
    r_q, r_r, rank_ok, _ = qr_ratios(f, o_q)
    b_q = BOUNDS["c_q"]
    r_f, r_p, pdec, _ = plane_ratios(f, o_p, b_q)
    r_c, r_l, r_d, r_t, ldec, _ = line_ratios(f, o_l)
    en, ef, qn, qf, ln, lf = f["eig3_families"], f["eig3_fam"], f["qr_families"], f["qr_fam"], f["line_families"], f["line_fam"]
    ratios = {"c_e": by_family(en, ef, r_e), "c_v": by_family(en, ef, r_v), "c_o": by_family(en, ef, r_o),
              "c_q": by_family(qn, qf, r_q), "c_r": by_family(qn, qf, r_r), "c_f": by_family(qn, qf, r_f),
              "c_p": by_family(qn, qf, r_p), "c_c": by_family(ln, lf, r_c), "c_l": by_family(ln, lf, r_l),
              "c_d": by_family(ln, lf, r_d), "c_t": by_family(ln, lf, r_t)}
    flags = {"eig3 order": ordered, "qr rank": rank_ok, "plane gate": pdec, "line gate": ldec,
             "eig3 finite": np.isfinite(o_e).all(1)}
    return ratios, flags
