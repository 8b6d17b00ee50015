"""Shared by tests/golden/make_undistort_kat.py (the generator), tests/test_undistort_kat.py (the oracle, CPU) and
tests/test_gpu_undistort_kat.py (the device): the known answers of RemoveLidarDistortion in tests/golden/undistort_kat.npz.

The reference of every comparison is `sequence`: the formula sequence of oracle/estimate.cpp:mmlo_undistort -- matrix -> quaternion
with Eigen's branch rules, normalized(), slerp from the identity (linear branch for |d| >= 1 - eps, sign flip for d < 0),
normalized(), q * v, + s dt, - dt, dR^T * -- evaluated on the doubles dR, dt and the floats x, y, z, s in a number type far wider
than double: numpy.longdouble (64-bit mantissa) to mine the points, mpmath at 50 digits to confirm every stored one; the two agree
to 1e-18 * scale.  scale = |x| + |y| + |z| + |dt|_1 is the kernel's own (undistort_point's `tol`).  Because the same sequence is
followed, a dR that is not exactly orthonormal has one defined answer too.

What is stored per point is the float that exact value rounds to and, per coordinate, `margin`: the distance of the exact value to
the nearest float rounding boundary (the midpoints between adjacent floats), divided by scale.  An implementation whose double
result is within margin * scale of the exact value rounds to the stored float; so the comparison is BIT EQUALITY.

B = 1.075e-15 (stored as `B` in the fixture; measured, not chosen): the largest |oracle's double result - exact| / scale over the
117.6 million candidates (352.8 million coordinates) the generator evaluated; 1.9e-16 for the identity, 4e-16 .. 5e-16 for the
rotations up to 2 rad, 7e-16 .. 1.1e-15 for those of 120 .. 180 degrees.  The oracle's double result is `oracle_double` below,
whose float rounding is asserted equal to mmlo_undistort's on every candidate; that float differs from the exact value's at 9 of the
coordinates, each within 2.8e-16 of a boundary.  No stored coordinate has margin < 8 B (such points were redrawn): the device's
exact path is the same operation count with another libm, a few ulp apart at worst.  The guard set of every motion holds points
with a coordinate at margin in [8 B, 5e-14]: inside the band (1e-13) in which the device must not trust its fast form.  (With the
fast form's own error near B the guard set cannot tell a guard that never fires from one that does; it tells a fast form, a band
or an exact path that is off by more than the margins, 8.6e-15 .. 5e-14.)
"""
import math
import os

import numpy as np

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "undistort_kat.npz")
ONE = 1.0 - 2.0 ** -52          # slerp's linear-branch threshold: 1 - NumTraits<double>::epsilon()
GUARD_HI = 5e-14                # upper end of the guard set's margins
DEVICE_BAND = 1e-13             # undistort_point's band (csrc/undistort_dev.h)
DECIDABLE = 8.0                 # x B
# quat_branch: which rule of Eigen's matrix -> quaternion assignment a motion takes
TRACE_POS, DIAG0, DIAG1, DIAG2 = range(4)


class LD:
    """numpy.longdouble, scalars or arrays"""
    num = staticmethod(lambda v: np.asarray(v, dtype=np.longdouble))
    sqrt, sin, acos = staticmethod(np.sqrt), staticmethod(np.sin), staticmethod(np.arccos)


def MP(dps=50):
    import mpmath as mp
    mp.mp.dps = dps

    class _MP:
        """mpmath, scalars"""
        num = staticmethod(lambda v: mp.mpf(float(v)))
        sqrt, sin, acos = staticmethod(mp.sqrt), staticmethod(mp.sin), staticmethod(mp.acos)
    return _MP


def motion_quat(A, dR):
    """Quaterniond(dR).normalized() in the number type A: (x, y, z, w), quat_branch"""
    m = [A.num(v) for v in np.asarray(dR, np.float64).reshape(9)]
    t = m[0] + m[4] + m[8]
    if t > 0:
        t = A.sqrt(t + 1)
        w = t / 2
        t = 1 / (2 * t)
        q = [(m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t, w]
        branch = TRACE_POS
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = A.sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1)
        q = [None] * 4
        q[i] = t / 2
        t = 1 / (2 * t)
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t
        branch = DIAG0 + i
    n = A.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [c / n for c in q], branch


def sequence(A, dR, dt, x, y, z, s):
    """The reference's formula sequence in the number type A.  x, y, z, s: what A.num made of the floats (arrays for LD).
    -> (px, py, pz), dict(quat_branch, linear, w_negative, theta)"""
    (qx, qy, qz, qw), branch = motion_quat(A, dR)
    m = [A.num(v) for v in np.asarray(dR, np.float64).reshape(9)]
    d = [A.num(v) for v in np.asarray(dt, np.float64).reshape(3)]
    absD = abs(qw)
    linear = bool(absD >= A.num(ONE))
    theta = A.num(0.0)
    if linear:
        scale0, scale1 = 1 - s, s
    else:
        theta = A.acos(absD)
        sin_theta = A.sin(theta)
        scale0 = A.sin((1 - s) * theta) / sin_theta
        scale1 = A.sin(s * theta) / sin_theta
    if qw < 0:
        scale1 = -scale1
    ax, ay, az, aw = scale1 * qx, scale1 * qy, scale1 * qz, scale0 + scale1 * qw
    n = A.sqrt(ax * ax + ay * ay + az * az + aw * aw)
    ax, ay, az, aw = ax / n, ay / n, az / n, aw / n
    ux, uy, uz = 2 * (ay * z - az * y), 2 * (az * x - ax * z), 2 * (ax * y - ay * x)
    rx = x + aw * ux + (ay * uz - az * uy)
    ry = y + aw * uy + (az * ux - ax * uz)
    rz = z + aw * uz + (ax * uy - ay * ux)
    vx, vy, vz = rx + s * d[0] - d[0], ry + s * d[1] - d[1], rz + s * d[2] - d[2]
    out = (m[0] * vx + m[3] * vy + m[6] * vz, m[1] * vx + m[4] * vy + m[7] * vz, m[2] * vx + m[5] * vy + m[8] * vz)
    return out, dict(quat_branch=branch, linear=linear, w_negative=bool(qw < 0), theta=float(theta))


def scale_of(xyz, dt):
    return np.abs(np.asarray(xyz, np.float64)).sum(-1) + float(np.abs(np.asarray(dt, np.float64)).sum())


def exact_ld(dR, dt, xyz, s):
    """`sequence` in numpy.longdouble on (n, 3) float32 points / (n,) float32 times -> (n, 3) longdouble, info"""
    xyz = np.asarray(xyz, np.float32)
    out, info = sequence(LD, dR, dt, LD.num(xyz[:, 0]), LD.num(xyz[:, 1]), LD.num(xyz[:, 2]), LD.num(np.asarray(s, np.float32)))
    return np.stack(out, 1), info


def exact_mp(A, dR, dt, p, s):
    """`sequence` in mpmath on one point -> [px, py, pz] (mpf), info"""
    out, info = sequence(A, dR, dt, A.num(p[0]), A.num(p[1]), A.num(p[2]), A.num(s))
    return list(out), info


def margins_ld(v, scale):
    """v: (n, 3) longdouble exact values -> (float32 roundings, margins (n, 3) float64).  A float keeps 24 significant bits: in the
    binade [2^(e-1), 2^e) of |v| the floats are 2^(e-24) apart and the boundaries sit half-way between them.  (A value just above a
    power of two has a nearer boundary below it, a quarter of this spacing away: never near, so never of interest here.)  Values
    below the normal float range get margin 0: never decidable, as the kernel never calls them safe."""
    a = np.abs(v)
    _, e = np.frexp(a)
    u = np.ldexp(np.longdouble(1), e - 24)
    r = a / u
    dist = np.abs(r - np.floor(r) - np.longdouble(0.5)) * u
    mg = np.where(a < np.longdouble(2.0) ** -126, 0, dist / LD.num(scale)[:, None]).astype(np.float64)
    return v.astype(np.float32), mg


def margin_mp(A, v, scale):
    """one exact mpf value -> (float32 rounding, margin as mpf)"""
    import mpmath as mp
    a = abs(v)
    if a < mp.mpf(2) ** -126:
        return np.float32(0.0), mp.mpf(0)
    _, e = mp.frexp(a)
    u = mp.ldexp(mp.mpf(1), e - 24)
    r = a / u
    k = mp.floor(r)
    dist = abs(r - k - mp.mpf(0.5)) * u
    f = (k if r - k < mp.mpf(0.5) else k + 1) * u      # (a tie would have margin 0: never stored)
    return np.float32(float(f if v > 0 else -f)), dist / A.num(scale)


def _glibc(f, a):
    return np.fromiter(map(f, a), np.float64, len(a))


def oracle_double(dR, dt, xyz, s):
    """oracle/estimate.cpp:mmlo_undistort restated operation for operation on IEEE doubles, BEFORE its rounding to float: numpy's
    + - * / and sqrt are the correctly rounded ones, sin and acos are the C library's (math.*), nothing is fused.  -> (n, 3) float64"""
    m = [float(v) for v in np.asarray(dR, np.float64).reshape(9)]
    d = [float(v) for v in np.asarray(dt, np.float64).reshape(3)]
    t = m[0] + m[4] + m[8]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        q = [(m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t, w]
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0)
        q = [0.0] * 4
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t
    n = math.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))
    qx, qy, qz, qw = q[0] / n, q[1] / n, q[2] / n, q[3] / n
    dd = (0.0 * qx + 0.0 * qz) + (0.0 * qy + 1.0 * qw)
    xyz = np.asarray(xyz, np.float32).astype(np.float64)
    sf = np.asarray(s, np.float32)
    tt = sf.astype(np.float64)
    if abs(dd) >= ONE:
        scale0, scale1 = 1.0 - tt, tt
    else:
        theta = math.acos(abs(dd))
        sin_theta = math.sin(theta)
        scale0 = _glibc(math.sin, (1.0 - tt) * theta) / sin_theta
        scale1 = _glibc(math.sin, tt * theta) / sin_theta
    if dd < 0.0:
        scale1 = -scale1
    ax, ay, az, aw = scale0 * 0.0 + scale1 * qx, scale0 * 0.0 + scale1 * qy, scale0 * 0.0 + scale1 * qz, scale0 * 1.0 + scale1 * qw
    n = np.sqrt((ax * ax + az * az) + (ay * ay + aw * aw))
    ax, ay, az, aw = ax / n, ay / n, az / n, aw / n
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    ux, uy, uz = ay * z - az * y, az * x - ax * z, ax * y - ay * x
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx, cy, cz = ay * uz - az * uy, az * ux - ax * uz, ax * uy - ay * ux
    px, py, pz = ((x + aw * ux) + cx) + tt * d[0], ((y + aw * uy) + cy) + tt * d[1], ((z + aw * uz) + cz) + tt * d[2]
    vx, vy, vz = px - d[0], py - d[1], pz - d[2]
    return np.stack([(m[0] * vx + m[3] * vy) + m[6] * vz, (m[1] * vx + m[4] * vy) + m[7] * vz, (m[2] * vx + m[5] * vy) + m[8] * vz], 1)


def load():
    z = np.load(KAT)
    f = {k: z[k] for k in z.files}
    f["B"] = float(f["B"])
    f["names"] = [str(n) for n in f["names"]]
    return f


def of_motion(f, m):
    """indices of motion m's points, random set first, in stored order"""
    return np.flatnonzero(f["motion"] == m)


def differing(f, got, idx=None):
    """got: (n, 3) float32 for the points idx (default: all).  -> the rows whose bits differ from the fixture's floats"""
    idx = np.arange(len(f["xyz"])) if idx is None else idx
    got = np.ascontiguousarray(got, np.float32)
    return idx[(got.view(np.uint32) != np.ascontiguousarray(f["ref"][idx]).view(np.uint32)).any(1)]


def report(f, got, idx, bad, what, worst=8):
    """The worst offenders among the rows `bad` (indices into the fixture; got is aligned with idx): motion, branch, s, the margin
    of the differing coordinate, and whether that put the point into the device's band or the guard set."""
    pos = {int(i): k for k, i in enumerate(idx)}
    rows = []
    for i in bad:
        g, r = got[pos[int(i)]], f["ref"][i]
        c = int(np.argmax(g.view(np.uint32) != r.view(np.uint32)))
        rows.append((f["margin"][i, c], int(i), c, g, r))
    rows.sort(key=lambda r: -r[0])
    lines = ["%s: %d of %d points differ from the exact reference's floats; largest margins first" % (what, len(bad), len(idx))]
    for mg, i, c, g, r in rows[:worst]:
        m = int(f["motion"][i])
        lines.append("  point %d motion %d (%s: quat branch %d, linear %d, w<0 %d, theta %.6g) %s set s=%.9g xyz=%r coordinate %d: got %r "
                     "want %r (%d ulp), margin %.3g (min over the point %.3g): %s the device's 1e-13 band"
                     % (i, m, f["names"][m], f["quat_branch"][m], f["linear"][m], f["w_negative"][m], f["theta"][m],
                        "guard" if f["guard"][i] else "random", f["s"][i], f["xyz"][i].tolist(), c, g[c], r[c],
                        int(g.view(np.int32)[c]) - int(r.view(np.int32)[c]), mg, f["margin"][i].min(),
                        "inside" if f["margin"][i].min() < DEVICE_BAND else "outside"))
    return "\n".join(lines)


def assert_bits(f, got, idx, what):
    bad = differing(f, got, idx)
    assert len(bad) == 0, report(f, np.ascontiguousarray(got, np.float32), idx, bad, what)
