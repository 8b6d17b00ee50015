"""Known answers for the IMU side of the full-window estimator, computed from the DEFINITIONS at 80 digits (mpmath), never from
the project's formulas:

    exp    the matrix exponential of the hat matrix (its closed form, Rodrigues, evaluated at 80 digits)
    log    its inverse with the angle in [0, pi]: theta = atan2(|v|, (tr - 1) / 2), v = vee(R - R') / 2, log = theta v / |v|
    r      Cost_NavState_PRV_Bias as include/mmloam_hip.h documents it, before the square-root information:
           rP = Ri'(Pj - Pi - Vi dt - g dt^2 / 2) - (dp + Jpbg dbg + Jpba dba),  rR = log((dR exp(Jrbg dbg))' Ri' Rj),
           rV = Ri'(Vj - Vi - g dt) - (dv + Jvbg dbg + Jvba dba),  the bias differences;  dR = the matrix of dq / |dq|
    J      the plain derivative of r in the 30 stored parameters [pr_i | vb_i | pr_j | vb_j], rotation vectors included, by
           central differences with step 1e-24 at 80 digits: no Jr or Jr^-1 formula anywhere
    U      chol(cov^-1)' of a covariance given in doubles, inverse and factor at 80 digits
    pre    the recurrence of IMUIntegrator::PreIntegration in exact arithmetic; its right Jacobian is the definition
           Jr(w) = int_0^1 exp(-s [w]x) ds summed as a power series, and the reference's DECISION Jr = I for |gyr dt| <= 1e-5 is
           taken as written
    prior  dx = [x - x0 | log(exp(x)^-1 exp(x0)) | x - x0], g = dx and cost = |dx|^2 / 2 for J = I, r0 = 0

Every value is rounded to double once.  Data only: tests/golden/imu_kat.npz.

    python tests/golden/make_imu_kat.py [seed [path]]

Sections (tests/imu_checks.py holds the units and the samples of the intervals, which are a formula, not data):
    f_*   raw factor items with covariance = I            p_*   pre-integrated intervals (imu_checks.INTERVALS)
    w_*   whitening: covariances of p_*, their exact U    d_*   prior items
"""
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import imu_checks as K  # noqa: E402  (the interval samples and the ladders: inputs, never results)

mp.mp.dps = 80
STEP = mp.mpf(10) ** -24
GRAV = np.array([0.0, 0.0, -9.805])
ZERO, ONE = mp.mpf(0), mp.mpf(1)


# ---- exact small dense arithmetic -------------------------------------------------------------------------------------------
def mpv(a):
    return [mp.mpf(float(v)) for v in np.asarray(a, float).reshape(-1)]


def mpm(a):
    return [mpv(row) for row in np.asarray(a, float)]


def fl(v):
    return [float(t) for t in v]


def eye():
    return [[ONE if r == c else ZERO for c in range(3)] for r in range(3)]


def mul(A, B):
    return [[sum(A[r][k] * B[k][c] for k in range(len(B))) for c in range(len(B[0]))] for r in range(len(A))]


def tr(A):
    return [list(c) for c in zip(*A)]


def mv(A, v):
    return [sum(a * b for a, b in zip(row, v)) for row in A]


def hat(v):
    return [[ZERO, -v[2], v[1]], [v[2], ZERO, -v[0]], [-v[1], v[0], ZERO]]


def exp_so3(w):
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2 == 0:
        return eye()
    th = mp.sqrt(th2)
    A, B = mp.sin(th) / th, (1 - mp.cos(th)) / th2
    Kx = hat(w)
    K2 = mul(Kx, Kx)
    return [[(ONE if r == c else ZERO) + A * Kx[r][c] + B * K2[r][c] for c in range(3)] for r in range(3)]


def log_so3(R):
    v = [(R[2][1] - R[1][2]) / 2, (R[0][2] - R[2][0]) / 2, (R[1][0] - R[0][1]) / 2]
    s = mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if s == 0:
        return [ZERO, ZERO, ZERO]
    th = mp.atan2(s, (R[0][0] + R[1][1] + R[2][2] - 1) / 2)
    return [th * t / s for t in v]


def quat_matrix(q):
    """the rotation of q / |q| (x, y, z, w)"""
    n = mp.sqrt(sum(t * t for t in q))
    x, y, z, w = [t / n for t in q]
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def matrix_quat(R):
    """(x, y, z, w) with w >= 0 of an exactly orthogonal R, through its largest component"""
    t = [1 + R[0][0] - R[1][1] - R[2][2], 1 - R[0][0] + R[1][1] - R[2][2], 1 - R[0][0] - R[1][1] + R[2][2], 1 + R[0][0] + R[1][1] + R[2][2]]
    i = max(range(4), key=lambda k: t[k])
    s = 2 * mp.sqrt(t[i])
    if i == 3:
        q = [(R[2][1] - R[1][2]) / s, (R[0][2] - R[2][0]) / s, (R[1][0] - R[0][1]) / s, s / 4]
    else:
        j, k = (i + 1) % 3, (i + 2) % 3
        q = [ZERO] * 4
        q[i], q[j], q[k], q[3] = s / 4, (R[j][i] + R[i][j]) / s, (R[k][i] + R[i][k]) / s, (R[k][j] - R[j][k]) / s
    return [-t_ for t_ in q] if q[3] < 0 else q


def right_jacobian_series(w):
    """int_0^1 exp(-s K) ds = sum (-K)^k / (k + 1)!, K = [w]x; with K^3 = -theta^2 K the sum is I - a K + b K^2,
    a = sum (-theta^2)^k / (2k + 2)!, b = sum (-theta^2)^k / (2k + 3)!: series, no cancellation"""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    a = b = ZERO
    term, k = ONE, 0
    while abs(term) > mp.mpf(10) ** -90:
        a += term / mp.factorial(2 * k + 2)
        b += term / mp.factorial(2 * k + 3)
        term *= -th2
        k += 1
    Kx = hat(w)
    K2 = mul(Kx, Kx)
    return [[(ONE if r == c else ZERO) - a * Kx[r][c] + b * K2[r][c] for c in range(3)] for r in range(3)]


# ---- the exact factor -------------------------------------------------------------------------------------------------------
def residual(x, pre, g):
    """x: 30 mpf; pre: dict of mpf lists (dp, dv, dR 3x3, dt, bg, ba, Jpbg, Jpba, Jrbg, Jvbg, Jvba)"""
    Pi, wi, Vi, bgi, bai = x[0:3], x[3:6], x[6:9], x[9:12], x[12:15]
    Pj, wj, Vj, bgj, baj = x[15:18], x[18:21], x[21:24], x[24:27], x[27:30]
    dt = pre["dt"]
    RiT = tr(exp_so3(wi))
    Rj = exp_so3(wj)
    dbg = [bgi[k] - pre["bg"][k] for k in range(3)]
    dba = [bai[k] - pre["ba"][k] for k in range(3)]
    a = [Pj[k] - Pi[k] - Vi[k] * dt - g[k] * dt * dt / 2 for k in range(3)]
    b = [Vj[k] - Vi[k] - g[k] * dt for k in range(3)]
    Ra, Rb = mv(RiT, a), mv(RiT, b)
    t1, t2 = mv(pre["Jpbg"], dbg), mv(pre["Jpba"], dba)
    rP = [Ra[k] - (pre["dp"][k] + t1[k] + t2[k]) for k in range(3)]
    t1, t2 = mv(pre["Jvbg"], dbg), mv(pre["Jvba"], dba)
    rV = [Rb[k] - (pre["dv"][k] + t1[k] + t2[k]) for k in range(3)]
    C = mul(pre["dR"], exp_so3(mv(pre["Jrbg"], dbg)))
    E = mul(tr(C), mul(RiT, Rj))
    rR = log_so3(E)
    return rP + rR + rV + [bgj[k] - bgi[k] for k in range(3)] + [baj[k] - bai[k] for k in range(3)], E


def exact_factor(x, pre, jac=True):
    xm = mpv(x)
    pm = dict(dp=mpv(pre["dp"]), dv=mpv(pre["dv"]), dR=quat_matrix(mpv(pre["dq"])), dt=mp.mpf(float(pre["dt"])), bg=mpv(pre["bg"]),
              ba=mpv(pre["ba"]), **{k: mpm(pre[k]) for k in ("Jpbg", "Jpba", "Jrbg", "Jvbg", "Jvba")})
    g = mpv(GRAV)
    r, E = residual(xm, pm, g)
    J = [[ZERO] * 30 for _ in range(15)]
    if jac:
        for c in range(30):
            xp, xn = list(xm), list(xm)
            xp[c] += STEP
            xn[c] -= STEP
            rp, rn = residual(xp, pm, g)[0], residual(xn, pm, g)[0]
            for q in range(15):
                J[q][c] = (rp[q] - rn[q]) / (2 * STEP)
    return r, J, E


def quat_branch(E):
    """the branch Eigen's matrix -> quaternion takes on E: 0 trace > 0, 1 + i the largest diagonal element otherwise"""
    if E[0][0] + E[1][1] + E[2][2] > 0:
        return 0
    i = 0
    if E[1][1] > E[0][0]:
        i = 1
    if E[2][2] > E[i][i]:
        i = 2
    return 1 + i


def half_angle_qw(E):
    """|qw| = cos(theta / 2) and n = sin(theta / 2) of the rotation E"""
    w = log_so3(E)
    th = mp.sqrt(sum(t * t for t in w))
    return mp.cos(th / 2), mp.sin(th / 2)


# ---- the exact pre-integration ----------------------------------------------------------------------------------------------
NOISE = [mp.mpf(K.GYR_N) ** 2] * 3 + [mp.mpf(K.ACC_N) ** 2] * 3 + [mp.mpf(K.GYR_W) ** 2] * 3 + [mp.mpf(K.ACC_W) ** 2] * 3


def apply_A(X, blk, dt):
    """A X for the A of one sample: identity plus the blocks (0,3) (0,6) (0,12) (3,3) (3,9) (6,3) (6,12)"""
    A03, A012, A33, A39, A63, A612 = blk
    n = len(X[0])
    out = [None] * 15
    for r in range(3):
        out[r] = [X[r][c] + sum(A03[r][j] * X[3 + j][c] for j in range(3)) + dt * X[6 + r][c] + sum(A012[r][j] * X[12 + j][c] for j in range(3)) for c in range(n)]
        out[3 + r] = [sum(A33[r][j] * X[3 + j][c] for j in range(3)) + sum(A39[r][j] * X[9 + j][c] for j in range(3)) for c in range(n)]
        out[6 + r] = [sum(A63[r][j] * X[3 + j][c] for j in range(3)) + X[6 + r][c] + sum(A612[r][j] * X[12 + j][c] for j in range(3)) for c in range(n)]
    for r in range(9, 15):
        out[r] = list(X[r])
    return out


def exact_preintegration(samples, bg, ba):
    bg, ba = mpv(bg), mpv(ba)
    R = eye()
    dp, dv, dtime = [ZERO] * 3, [ZERO] * 3, ZERO
    jac = [[ONE if r == c else ZERO for c in range(15)] for r in range(15)]
    cov = [[ZERO] * 15 for _ in range(15)]
    gnorm = mp.mpf(K.GNORM)
    above = 0
    for m in samples:
        m = mpv(m)
        gyr = [m[k] - bg[k] for k in range(3)]
        acc = [m[3 + k] * gnorm - ba[k] for k in range(3)]
        dt = m[6]
        dt2 = dt * dt
        gdt = [t * dt for t in gyr]
        dR = exp_so3(gdt)
        nrm = mp.sqrt(sum(t * t for t in gdt))
        Jr = eye()
        if nrm > mp.mpf("0.00001"):                           # the reference's decision, as written
            Jr = right_jacobian_series(gdt)
            above += 1
        RA = mul(R, hat(acc))
        sc = lambda M, s: [[s * t for t in row] for row in M]
        blk = (sc(RA, -dt2 / 2), sc(R, -dt2 / 2), tr(dR), sc(Jr, -dt), sc(RA, -dt), sc(R, -dt))
        jac = apply_A(jac, blk, dt)
        T = apply_A(cov, blk, dt)
        cov = tr(apply_A(tr(T), blk, dt))
        # B noise B': B rows 0-2 dt2/2 R (cols 3-5), 3-5 dt Jr (cols 0-2), 6-8 dt R (cols 3-5), 9-14 dt
        Bp, Br, Bv = sc(R, dt2 / 2), sc(Jr, dt), sc(R, dt)
        rows = {0: Bp, 6: Bv}
        for r0, Ba in rows.items():
            for c0, Bb in rows.items():
                for r in range(3):
                    for c in range(3):
                        cov[r0 + r][c0 + c] += NOISE[3] * sum(Ba[r][j] * Bb[c][j] for j in range(3))
        for r in range(3):
            for c in range(3):
                cov[3 + r][3 + c] += NOISE[0] * sum(Br[r][j] * Br[c][j] for j in range(3))
        for r in range(9, 15):
            cov[r][r] += dt2 * NOISE[r - 3]
        Racc = mv(R, acc)
        dp = [dp[k] + dv[k] * dt + Racc[k] * dt2 / 2 for k in range(3)]
        dv = [dv[k] + Racc[k] * dt for k in range(3)]
        R = mul(R, dR)
        dtime += dt
    th = log_so3(R)
    return dict(dp=fl(dp), dv=fl(dv), dq=fl(matrix_quat(R)), dtime=float(dtime), jacobian=[fl(r) for r in jac], covariance=[fl(r) for r in cov],
                above=above, angle=float(mp.sqrt(sum(t * t for t in th))))


def exact_sqrt_info(cov):
    """-> U = chol(cov^-1)' (15 x 15 upper), the condition number of cov in the 2-norm and that of the covariance scaled to a unit
    diagonal (what an inverse through a Cholesky factor sees)"""
    A = mp.matrix(mpm(cov))
    inv = A ** -1
    inv = (inv + inv.T) / 2
    L = mp.cholesky(inv)
    U = L.T
    d = np.sqrt(np.diag(cov))
    sv = lambda M: np.linalg.svd(M, compute_uv=False)
    s2, ss = sv(np.asarray(cov, float)), sv(np.asarray(cov, float) / np.outer(d, d))
    return U, [[float(U[r, c]) for c in range(15)] for r in range(15)], s2[0] / s2[-1], ss[0] / ss[-1]


# ---- items ------------------------------------------------------------------------------------------------------------------
def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def rotvec_of(R):
    return np.array(fl(log_so3(R)))


def geometry(seed, k, dq=None):
    """geometry k: dt of 0.005, 0.1, 1; positions within 2 m, velocities within 3 m/s, O(1) residuals (sensitive rows)"""
    rng = np.random.default_rng([seed, 10, k])
    dt = K.DTS[k % 3]
    q = unit(rng) * np.sin(0.4) if dq is None else None
    g = dict(dt=dt, Pi=rng.uniform(-2, 2, 3), Vi=rng.uniform(-3, 3, 3), bgi=rng.normal(0, 0.01, 3), bai=rng.normal(0, 0.1, 3),
             dq=np.append(q, np.cos(0.4)) if dq is None else np.asarray(dq), dp=rng.uniform(-3, 3, 3) * dt, dv=rng.uniform(-10, 10, 3) * dt,
             u1=unit(rng), u2=unit(rng), u3=unit(rng), u4=unit(rng),
             Jpbg=rng.normal(0, 5, (3, 3)) * dt ** 3, Jvbg=rng.normal(0, 10, (3, 3)) * dt ** 2,
             Jpba=-0.5 * dt * dt * (np.eye(3) + rng.normal(0, 0.1, (3, 3))), Jvba=-dt * (np.eye(3) + rng.normal(0, 0.1, (3, 3))),
             Jrbg=-dt * (np.eye(3) + rng.normal(0, 0.1, (3, 3))), off=rng.uniform(-0.5, 0.5, 6), dbj=rng.normal(0, 1e-3, 6),
             dba=rng.normal(0, 0.05, 3))
    g["dq"] = g["dq"] / np.linalg.norm(g["dq"])
    return g


def make_item(g, wi, dbg, wj=None, rho=None):
    """-> (x30, pre).  wj, or rho: Rj = Ri C exp(rho) so that the rotation residual is rho (to the rounding of wj)"""
    pre = dict(dp=g["dp"], dv=g["dv"], dq=g["dq"], dt=g["dt"], bg=g["bgi"] - dbg, ba=g["bai"] - g["dba"],
               **{k: g[k] for k in ("Jpbg", "Jpba", "Jrbg", "Jvbg", "Jvba")})
    if wj is None:
        dbg_seen = mpv(g["bgi"])
        dbg_seen = [dbg_seen[k] - mp.mpf(float(pre["bg"][k])) for k in range(3)]
        C = mul(quat_matrix(mpv(pre["dq"])), exp_so3(mv(mpm(pre["Jrbg"]), dbg_seen)))
        wj = rotvec_of(mul(exp_so3(mpv(wi)), mul(C, exp_so3(mpv(rho)))))
    dt = g["dt"]
    Pj = g["Pi"] + g["Vi"] * dt + 0.5 * GRAV * dt * dt + g["dp"] + g["off"][:3]
    Vj = g["Vi"] + GRAV * dt + g["dv"] + g["off"][3:]
    x = np.concatenate([g["Pi"], wi, g["Vi"], g["bgi"], g["bai"], Pj, wj, Vj, g["bgi"] + g["dbj"][:3], g["bai"] + g["dbj"][3:]])
    return x, pre


def factor_families(seed):
    fam = {}
    G = [geometry(seed, k) for k in range(K.N_GEOM)]
    dbg0 = lambda g: 1e-3 * g["u3"]
    for name, th in K.LADDER_I:
        fam["thi_" + name] = [make_item(g, th * g["u1"], dbg0(g), wj=th * g["u2"]) for g in G]
    for name, th in K.LADDER_R:
        fam["thr_" + name] = [make_item(g, 0.7 * g["u1"], dbg0(g), rho=th * g["u2"]) for g in G]
    for name, d in K.NEAR_PI:
        fam["rpi_" + name] = [make_item(g, 0.7 * g["u1"], dbg0(g), rho=fl([(mp.pi - mp.mpf(d)) * mp.mpf(float(t)) for t in g["u2"]])) for g in G]
    for name, v in K.DBG:
        fam["dbg_" + name] = [make_item(g, 0.7 * g["u1"], v * g["u3"], wj=0.5 * g["u2"]) for g in G]
    for i, name in enumerate("xyz"):
        it = []
        for g in G:
            ax = 0.2 * g["u4"]
            ax[i] += 1.0
            it.append(make_item(g, 0.7 * g["u1"], dbg0(g), rho=2.8 * ax / np.linalg.norm(ax)))
        fam["quat_" + name] = it
    return fam


def whiten_items(seed, pres):
    """per covariance N_GEOM states around the pre-integration's own motion"""
    out = []
    for c, p in enumerate(pres):
        for k in range(K.N_GEOM):
            rng = np.random.default_rng([seed, 20, c, k])
            dt = p["dtime"]
            Pi, Vi, wi = rng.uniform(-2, 2, 3), rng.uniform(-3, 3, 3), 0.7 * unit(rng)
            Ri = np.array([fl(r) for r in exp_so3(mpv(wi))])
            bgi, bai = np.asarray(p["bg"]) + rng.normal(0, 1e-4, 3), np.asarray(p["ba"]) + rng.normal(0, 1e-3, 3)
            s = np.sqrt(np.diag(np.asarray(p["covariance"])))
            Pj = Pi + Vi * dt + 0.5 * GRAV * dt * dt + Ri @ np.asarray(p["dp"]) + 3 * s[0:3] * rng.normal(size=3)
            Vj = Vi + GRAV * dt + Ri @ np.asarray(p["dv"]) + 3 * s[6:9] * rng.normal(size=3)
            wj = rotvec_of(mul(exp_so3(mpv(wi)), mul(quat_matrix(mpv(p["dq"])), exp_so3(mpv(3 * s[3:6] * rng.normal(size=3))))))
            x = np.concatenate([Pi, wi, Vi, bgi, bai, Pj, wj, Vj, bgi + 3 * s[9:12] * rng.normal(size=3), bai + 3 * s[12:15] * rng.normal(size=3)])
            Jm = np.asarray(p["jacobian"])
            pre = dict(dp=p["dp"], dv=p["dv"], dq=p["dq"], dt=dt, bg=p["bg"], ba=p["ba"], Jpbg=Jm[0:3, 9:12], Jpba=Jm[0:3, 12:15],
                       Jrbg=Jm[3:6, 9:12], Jvbg=Jm[6:9, 9:12], Jvba=Jm[6:9, 12:15])
            out.append((c, x, pre))
    return out


def prior_items(seed):
    fam = {}
    for name, th in K.LADDER_R + [("pi-" + n, None) for n, _ in K.NEAR_PI]:
        it = []
        for k in range(K.N_GEOM):
            rng = np.random.default_rng([seed, 30, k])
            x = np.concatenate([rng.uniform(-2, 2, 3), 0.7 * unit(rng), rng.uniform(-3, 3, 3), rng.normal(0, 0.01, 3), rng.normal(0, 0.1, 3)])
            u = unit(rng)
            rho = [mp.mpf(float(th)) * mp.mpf(float(t)) for t in u] if th is not None else \
                [(mp.pi - mp.mpf(dict(K.NEAR_PI)[name[3:]])) * mp.mpf(float(t)) for t in u]
            x0 = x + np.concatenate([rng.uniform(-0.5, 0.5, 3), np.zeros(3), rng.uniform(-0.5, 0.5, 3), rng.normal(0, 1e-3, 6)])
            x0[3:6] = rotvec_of(mul(exp_so3(mpv(x[3:6])), exp_so3(rho)))
            it.append((x, x0))
        fam["d_" + name] = it
    return fam


def exact_prior(x, x0):
    xm, x0m = mpv(x), mpv(x0)
    E = mul(tr(exp_so3(xm[3:6])), exp_so3(x0m[3:6]))
    dx = [xm[k] - x0m[k] for k in range(3)] + log_so3(E) + [xm[k] - x0m[k] for k in range(6, 15)]
    qw, n = half_angle_qw(E)
    return fl(dx), float(sum(t * t for t in dx) / 2), float(qw), float(n), quat_branch(E)


def write_npz(path, arrays):
    """an .npz whose bytes depend on the arrays alone (fixed member times)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.asanyarray(a), allow_pickle=False)


PRE_KEYS = ("dp", "dv", "dq", "dt", "bg", "ba", "Jpbg", "Jpba", "Jrbg", "Jvbg", "Jvba")


def pack_factor_items(prefix, items, jac_flags):
    out = {prefix + "x": np.array([x for x, _ in items])}
    for k in PRE_KEYS:
        out[prefix + k] = np.array([p[k] for _, p in items], float)
    r, J, br, qw, qn, rm, Jm = [], [], [], [], [], [], []
    for (x, p), jf in zip(items, jac_flags):
        rr, JJ, E = exact_factor(x, p, jac=jf)
        rm.append(rr)
        Jm.append(JJ)
        r.append(fl(rr))
        J.append([fl(row) for row in JJ])
        br.append(quat_branch(E))
        a, b = half_angle_qw(E)
        qw.append(float(a))
        qn.append(float(b))
    out.update({prefix + "r": np.array(r), prefix + "J": np.array(J), prefix + "branch": np.array(br, np.int8), prefix + "qw": np.array(qw),
                prefix + "qn": np.array(qn), prefix + "has_J": np.array(jac_flags)})
    return out, rm, Jm


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 20261019
    out = dict(seed=np.int64(seed))
    # ---- (c) pre-integration: the intervals are imu_checks.INTERVALS, their samples imu_checks.interval_samples
    pres = []
    for spec in K.INTERVALS:
        smp, bg, ba = K.interval_samples(spec, seed)
        p = exact_preintegration(smp, bg, ba)
        p["bg"], p["ba"] = bg, ba
        pres.append(p)
        print("interval %-10s n %4d above 1e-5: %4d, total angle %.3f" % (spec["name"], spec["n"], p["above"], p["angle"]), flush=True)
    for k in ("dp", "dv", "dq", "dtime", "jacobian", "above", "angle"):
        out["p_" + k] = np.array([p[k] for p in pres])
    iu = np.triu_indices(15)
    out["p_cov"] = np.array([np.asarray(p["covariance"])[iu] for p in pres])
    # ---- (b) whitening
    wsel = [i for i, s in enumerate(K.INTERVALS) if s["name"].startswith("cov_")]
    wpre = [pres[i] for i in wsel]
    Ue, U, k2, ks = zip(*[exact_sqrt_info(np.asarray(p["covariance"])) for p in wpre])
    out.update(w_interval=np.array(wsel, np.int16), w_U=np.array(U), w_cond2=np.array(k2), w_cond=np.array(ks))
    print("condition numbers (2-norm, unit diagonal):", ["%.3g %.3g" % t for t in zip(k2, ks)], flush=True)
    items = whiten_items(seed, wpre)
    packed, r, J = pack_factor_items("w_", [(x, p) for _, x, p in items], [True] * len(items))
    cidx = [c for c, _, _ in items]
    packed["w_cov"] = np.array(cidx, np.int8)
    rw, Jw = [], []                           # U at 80 digits times the raw values at 80 digits, rounded once
    for c, rr, JJ in zip(cidx, r, J):
        rw.append([float(sum(Ue[c][i, k] * rr[k] for k in range(i, 15))) for i in range(15)])
        Jw.append([[float(sum(Ue[c][i, k] * JJ[k][cc] for k in range(i, 15))) for cc in range(30)] for i in range(15)])
    packed["w_rw"], packed["w_Jw"] = np.array(rw), np.array(Jw)
    for k in ("w_dp", "w_dv", "w_dq", "w_dt", "w_bg", "w_ba", "w_Jpbg", "w_Jpba", "w_Jrbg", "w_Jvbg", "w_Jvba"):
        del packed[k]                          # the records are p_* of w_interval
    out.update(packed)
    # ---- (a) raw factor
    fam = factor_families(seed)
    names = list(fam)
    items = [it for n in names for it in fam[n]]
    flags = [not n.startswith("rpi_") for n in names for _ in fam[n]]
    packed, _, _ = pack_factor_items("f_", items, flags)
    out.update(packed)
    out.update(f_families=np.array(names), f_fam=np.array([i for i, n in enumerate(names) for _ in fam[n]], np.int16))
    # ---- (d) prior
    pf = prior_items(seed)
    pn = list(pf)
    ex = [exact_prior(x, x0) for n in pn for x, x0 in pf[n]]
    out.update(d_families=np.array(pn), d_fam=np.array([i for i, n in enumerate(pn) for _ in pf[n]], np.int16),
               d_x=np.array([x for n in pn for x, _ in pf[n]]), d_x0=np.array([x0 for n in pn for _, x0 in pf[n]]),
               d_dx=np.array([e[0] for e in ex]), d_cost=np.array([e[1] for e in ex]), d_qw=np.array([e[2] for e in ex]),
               d_qn=np.array([e[3] for e in ex]), d_branch=np.array([e[4] for e in ex], np.int8))
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "imu_kat.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes; factor items %d, intervals %d, whitening items %d, prior items %d" %
          (len(items), len(pres), len(cidx), len(ex)))


if __name__ == "__main__":
    main()
