"""mml_velo_fov_select[_batch] without a device: the NULL-context host path (csrc/velo_fov.h) against an independent restatement
of velo_cloud_handler's loop (unionLidarsAligner.cpp:437-490), to the byte -- rows, counts, startOri, endOri and the point that
set halfPassed.  The restatement below is a plain sequential loop over numpy.float32 / Python float written from the
statements of the reference, and never calls the library.  Its atan2f is glibc's own, called through ctypes: numpy.arctan2 on
float32 operands is NOT that function on every machine (on an AVX-512 host numpy dispatches to a vector routine that differs from
glibc's atan2f in the last bit for about 40 % of a scan's points), and glibc's is what the reference binary calls and what
csrc/libm_f32.h is pinned to (tests/test_host.py::test_libm_f32_equals_glibc).
What the device computes is tests/test_gpu_velo_fov.py, which compares it with the host path checked here."""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

F = np.float32
PI = math.pi

_libm = C.CDLL("libm.so.6")
_libm.atan2f.restype = C.c_float
_libm.atan2f.argtypes = [C.c_float, C.c_float]


def atan2f(y, x):
    """glibc's atan2f, element by element: float32 arrays in, float32 array out."""
    return np.array([_libm.atan2f(C.c_float(a), C.c_float(b)) for a, b in zip(y, x)], np.float32).reshape(-1)


def restate(pts):
    """velo_cloud_handler :437-490 for one frame (n, >= 3) float32.  Returns (rows (k, 4) float32, info tuple (startOri, endOri, h,
    kept), hits = the set of branches / predicate clauses taken)."""
    pts = np.asarray(pts, np.float32)
    n = len(pts)
    hits = set()
    if n == 0:                                           # (the reference reads points[0]; the library defines: nothing)
        return np.zeros((0, 4), np.float32), (F(0), F(0), -1, 0), hits
    with np.errstate(all="ignore"):
        A = -atan2f(pts[:, 1], pts[:, 0])
        assert A.dtype == np.float32
        startOri = F(A[0])
        endOri = F(float(A[n - 1]) + 2 * PI)
        if float(F(endOri - startOri)) > 3 * PI:
            endOri = F(float(endOri) - 2 * PI)
        elif float(F(endOri - startOri)) < PI:
            endOri = F(float(endOri) + 2 * PI)
        rows = []
        halfPassed = False
        h = -1
        for i in range(n):
            ori = F(A[i])
            if not halfPassed:
                hits.add("first")
                if float(ori) < float(startOri) - PI / 2:
                    ori = F(float(ori) + 2 * PI)
                elif float(ori) > float(startOri) + PI * 3 / 2:
                    ori = F(float(ori) - 2 * PI)
                if float(F(ori - startOri)) > PI:
                    halfPassed = True
                    h = i
            else:
                hits.add("second")
                ori = F(float(ori) + 2 * PI)
                if float(ori) < float(endOri) - PI * 3 / 2:
                    ori = F(float(ori) + 2 * PI)
                elif float(ori) > float(endOri) + PI / 2:
                    ori = F(float(ori) - 2 * PI)
            relTime = F(F(ori - startOri) / F(endOri - startOri))
            o = float(ori)
            c1 = o > -0.7608 and o < 0.7158
            c2 = o > -0.7608 + 2 * PI and o < 0.7158 + 2 * PI
            if c1 or c2:
                hits.add("clause1" if c1 else "clause2")
                rows.append((pts[i, 0], pts[i, 1], pts[i, 2], relTime))
    out = np.array(rows, np.float32).reshape(-1, 4)
    return out, (startOri, endOri, h, len(rows)), hits


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_against_restatement(M, frames, out, want=None):
    """out: what velo_fov_select returned for `frames`; want: restate() of each (computed when not given)."""
    want = want if want is not None else [restate(f) for f in frames]
    at = 0
    for i, (rows, (s, e, h, k), _) in enumerate(want):
        info = out["info"][i]
        assert out["n_kept"][i] == k and info["n_kept"] == k, i
        assert same_bits(info["start_ori"], s) and same_bits(info["end_ori"], e), i
        assert info["half_index"] == h, i
        assert same_bits(out["xyzt"][at:at + k], rows), i
        at += k
    assert at == len(out["xyzt"]) == len(out["xyz"]) and out["offsets"][-1] == at
    assert same_bits(out["xyz"], out["xyzt"][:, :3])


def rotated_scan(synth, k, start_ori):
    """A reduced VLP-16 revolution (about 3 600 points) rotated about z so that its first point has -atan2(y, x) = start_ori."""
    v = synth.velo_scan_vlp16(k, n_firings=228, firing_step_scale=8.0)
    a = (-math.atan2(float(v[0, 1]), float(v[0, 0]))) - start_ori      # rotate by +a: atan2 grows by a, ori falls by a
    c, s = math.cos(a), math.sin(a)
    x = v[:, 0].astype(np.float64)
    y = v[:, 1].astype(np.float64)
    out = v.copy()
    out[:, 0] = (c * x - s * y).astype(np.float32)
    out[:, 1] = (s * x + c * y).astype(np.float32)
    return out


def ring(oris, seed=0):
    """Points with -atan2(y, x) = oris (radians, any real), at random ranges and heights: (n, 4) float32."""
    rng = np.random.default_rng(seed)
    o = np.asarray(oris, np.float64)
    r = rng.uniform(3.0, 30.0, len(o))
    return np.stack([r * np.cos(-o), r * np.sin(-o), rng.uniform(-2.0, 2.0, len(o)), rng.uniform(0, 255, len(o))], 1).astype(np.float32)


START_ORIS = (0.0, 0.7, -0.7, PI / 2, -PI / 2, PI)


def hand_frames():
    nan_mid = ring(np.linspace(-0.5, 5.6, 400), 5)
    nan_mid[200, :3] = np.nan
    nan_first = ring(np.linspace(-0.5, 5.6, 400), 6)
    nan_first[0, 0] = np.nan
    h_last = ring(np.concatenate([np.linspace(0.0, 3.0, 99), [3.3]]), 7)
    return {
        "n0": np.zeros((0, 4), np.float32),
        "n1": ring([0.2], 1),
        "n2": ring([0.2, 0.4], 2),
        "all_outside": ring(np.linspace(2.0, 2.5, 300), 3),
        "all_inside_h_never": ring(np.linspace(-0.5, 0.5, 300), 4),
        "h_last": h_last,
        "nan_mid": nan_mid,
        "nan_first": nan_first,
    }


@pytest.fixture(scope="module")
def cases(synth):
    frames = {("scan", s): rotated_scan(synth, 20 + i, s) for i, s in enumerate(START_ORIS)}
    frames.update(hand_frames())
    return {k: (f, restate(f)) for k, f in frames.items()}


def test_header_declares_and_library_exports_the_entry_points(M):
    header = open(M.HEADER_PATH).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH], text=True)
    assert re.search(r"\bint\s+mml_velo_fov_select_batch\s*\(\s*mml_ctx\s*\*\s*ctx", header)
    assert re.search(r"\bint\s+mml_velo_fov_select\s*\(\s*mml_ctx\s*\*", header)
    for name in ("mml_velo_fov_select_batch", "mml_velo_fov_select"):
        assert re.search(r"\bT %s$" % name, syms, re.M), name
    assert re.search(r"#define\s+MML_FOV_BATCH_MAX\s+%d\b" % M.FOV_BATCH_MAX, header) and M.FOV_BATCH_MAX == 65535
    assert re.search(r"#define\s+MML_ABI_VERSION\s+1\b", header) and M.lib().mml_abi_version() == 1
    assert M.VELO_FOV_INFO_DTYPE.itemsize == 16
    assert callable(M.Context.velo_fov_select) and callable(M.velo_fov_select) and callable(M.velo_fov_select_raw)
    src = open(M.LIB_PATH.replace("libmmloam_hip.so", "csrc/velo_fov.hip")).read()
    assert re.search(r"#define\s+VFOV_BLOCK\s+%d\b" % M.FOV_TILE_POINTS, src)
    assert re.search(r"#define\s+VFOV_REG_TILES\s+%d\b" % (M.FOV_REG_POINTS // M.FOV_TILE_POINTS), src)


def test_restatement_covers_every_branch(cases):
    """The frames do what they are meant to, by the restatement alone: every frame meant to be non-empty keeps points, both
    clauses of the predicate and both halfPassed branches are taken, FOV points lie at the start, the end, both ends or the middle."""
    hits = set()
    for key, (f, (rows, info, hh)) in cases.items():
        hits |= hh
        if key in ("n0", "all_outside"):
            assert info[3] == 0, key
        else:
            assert info[3] > 0, key
    assert hits == {"first", "second", "clause1", "clause2"}
    scan = {s: cases[("scan", s)] for s in START_ORIS}
    for s, (f, (rows, info, hh)) in scan.items():
        assert abs(float(info[0]) - s) < 1e-3 or abs(abs(float(info[0])) - PI) < 1e-3, s
        assert 0 < info[2] < len(f) - 1 and 100 < info[3] < len(f) // 2, s        # h in the middle, a real selection
    rel = lambda s: scan[s][1][0][:, 3]
    assert rel(0.0).min() < 0.15 and rel(0.0).max() > 0.85 and not np.any((rel(0.0) > 0.2) & (rel(0.0) < 0.8))     # both ends
    assert scan[0.0][1][2] == {"first", "second", "clause1", "clause2"}                                         # (the + 2 pi clause)
    assert np.mean(rel(0.7) > 0.7) > 0.95                     # startOri 0.7: the end of the sweep (and the first few points)
    assert np.mean(rel(-0.7) < 0.3) > 0.90                    # startOri -0.7: the start (and the last few points)
    for s in (PI / 2, -PI / 2, PI):
        assert rel(s).min() > 0.1 and rel(s).max() < 0.9, s                                                     # the middle
    assert cases["all_inside_h_never"][1][1][2] == -1 and cases["all_inside_h_never"][1][1][3] == 300
    assert cases["h_last"][1][1][2] == 99
    assert cases["n1"][1][1][3] == 1 and cases["n2"][1][1][3] == 2
    # A NaN first point: startOri is NaN, so no comparison against it holds -- no point is adjusted, none sets halfPassed, every
    # relTime is NaN -- but the predicate reads ori alone: the points whose unadjusted -atan2f lies in the first clause are still
    # kept.  The frame is NOT emptied; this is what the reference's statements do, and the library follows them.
    f, (rows, info, hh) = cases["nan_first"]
    raw = -np.arctan2(f[:, 1], f[:, 0]).astype(np.float64)
    assert np.isnan(info[0]) and info[2] == -1 and hh == {"first", "clause1"}
    assert info[3] == int(np.sum((raw > -0.7608) & (raw < 0.7158))) > 0 and np.all(np.isnan(rows[:, 3]))
    f, (rows, info, hh) = cases["nan_mid"]
    assert info[3] > 0 and not np.any(np.isnan(rows)) and 0 < info[2] < 399


def test_host_path_equals_the_restatement_frame_by_frame(M, cases):
    for key, (f, want) in cases.items():
        check_against_restatement(M, [f], M.velo_fov_select([f]), [want])


def test_batch_equals_the_single_calls(M, cases):
    keys = list(cases)
    frames = [cases[k][0] for k in keys]
    batch = M.velo_fov_select(frames)
    check_against_restatement(M, frames, batch, [cases[k][1] for k in keys])
    singles = [M.velo_fov_select([f]) for f in frames]
    assert batch["xyzt"].tobytes() == b"".join(s["xyzt"].tobytes() for s in singles)
    assert batch["xyz"].tobytes() == b"".join(s["xyz"].tobytes() for s in singles)
    assert batch["info"].tobytes() == b"".join(s["info"].tobytes() for s in singles)
    assert batch["n_kept"].tolist() == [int(s["n_kept"][0]) for s in singles]
    # the running sums of n_kept are the velo_offsets of the time-offset search
    lo = np.arange(len(frames) + 1, dtype=np.int32) * 0
    rc, bad, _ = M.time_offset_plan(batch["offsets"], lo, 30, 12000, max_map_points=1 << 21)
    assert rc == M.MML_OK and bad == -1
    assert batch["offsets"].dtype == np.int32 and batch["offsets"][0] == 0 and np.all(np.diff(batch["offsets"]) == batch["n_kept"])


def test_strided_records_equal_the_packed_points(M, cases):
    f = cases[("scan", 0.0)][0]
    packed = M.velo_fov_select([f])
    rec = np.full((len(f), 8), -77.0, np.float32)              # point_step 32: x at byte 4, y at 12, z at 20
    rec[:, 1], rec[:, 3], rec[:, 5] = f[:, 0], f[:, 1], f[:, 2]
    raw = np.concatenate([np.full(5, 9, np.uint8), rec.reshape(-1).view(np.uint8)])     # the frame starts at an odd byte
    out = M.velo_fov_select_raw(raw, [5], [len(f)], 32, 4, 12, 20)
    for k in ("xyzt", "xyz", "info", "n_kept"):
        assert out[k].tobytes() == packed[k].tobytes(), k
    # three floats per record, nothing else: point_step 12
    out = M.velo_fov_select_raw(np.ascontiguousarray(f[:, :3]).reshape(-1).view(np.uint8), [0], [len(f)], 12, 0, 4, 8)
    assert out["xyzt"].tobytes() == packed["xyzt"].tobytes()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class RawCall:
    """One direct call of the C entry point with sentinel-filled outputs."""

    def __init__(self, M, frames, cap=None, want=(True, True)):
        self.M = M
        self.data, self.bo, self.npts, self.step = M.velo_fov_pack(frames)
        self.n = len(frames)
        rows = max(sum(len(f) for f in frames), 1) if cap is None else max(cap, 1)
        self.cap = rows if cap is None else cap
        self.xyzt = np.full((rows, 4), -5.0, np.float32) if want[0] else None
        self.xyz = np.full((rows, 3), -5.0, np.float32) if want[1] else None
        self.kept = np.full(max(self.n, 1), -3, np.int32)
        self.info = np.full(max(self.n, 1) * 4, -3, np.int32)
        self.off = (0, 4, 8)

    def run(self, ctx=None, **over):
        a = dict(n=self.n, data=_p(self.data), bo=_p(self.bo), npts=_p(self.npts), step=self.step, ox=self.off[0], oy=self.off[1],
                 oz=self.off[2], xyzt=_p(self.xyzt), xyz=_p(self.xyz), cap=self.cap, kept=_p(self.kept), info=_p(self.info))
        a.update(over)
        return self.M.lib().mml_velo_fov_select_batch(ctx, a["n"], a["data"], a["bo"], a["npts"], a["step"], a["ox"], a["oy"], a["oz"],
                                                      a["xyzt"], a["xyz"], a["cap"], a["kept"], a["info"])

    def untouched(self):
        return ((self.xyzt is None or np.all(self.xyzt == -5.0)) and (self.xyz is None or np.all(self.xyz == -5.0))
                and np.all(self.kept == -3) and np.all(self.info == -3))


def test_sizing_call_and_capacity(M, cases):
    frames = [cases[("scan", 0.7)][0], cases["n0"][0], cases[("scan", PI)][0]]
    want = [cases[("scan", 0.7)][1][1][3], 0, cases[("scan", PI)][1][1][3]]
    c = RawCall(M, frames, want=(False, False))
    assert c.run(cap=-1) == M.MML_OK                         # both outputs NULL: capacity_rows is not read
    assert c.kept.tolist() == want
    assert c.info.reshape(-1, 4)[:, 3].tolist() == want
    total = sum(want)
    c = RawCall(M, frames, cap=total - 1)
    assert c.run() == M.MML_ERR_CAPACITY and c.untouched()
    c = RawCall(M, frames, cap=total)
    assert c.run() == M.MML_OK and c.kept.tolist() == want and not np.any(c.xyzt[:total] == -5.0)
    # one output alone
    d = RawCall(M, frames, cap=total, want=(False, True))
    assert d.run() == M.MML_OK and d.xyz[:total].tobytes() == c.xyz[:total].tobytes()
    # the single entry point is the n = 1 case
    f = frames[0]
    xyzt, kept, info = np.zeros((want[0], 4), np.float32), np.zeros(1, np.int32), np.zeros(1, M.VELO_FOV_INFO_DTYPE)
    raw = np.ascontiguousarray(f).reshape(-1).view(np.uint8)
    assert M.lib().mml_velo_fov_select(None, _p(raw), len(f), 16, 0, 4, 8, _p(xyzt), None, want[0], _p(kept), _p(info)) == M.MML_OK
    assert xyzt.tobytes() == c.xyzt[:want[0]].tobytes() and kept[0] == want[0] and info["n_kept"][0] == want[0]


def test_refusals_leave_the_outputs_untouched(M, cases):
    frames = [cases["n2"][0], cases["all_inside_h_never"][0]]
    inv = M.MML_ERR_INVALID
    bad = [dict(n=0), dict(n=-1), dict(n=M.FOV_BATCH_MAX + 1), dict(data=None), dict(bo=None), dict(npts=None), dict(kept=None),
           dict(step=11), dict(step=8), dict(ox=-4), dict(oy=14), dict(oz=13), dict(oz=2), dict(ox=16), dict(cap=-1)]
    for over in bad:
        c = RawCall(M, frames)
        assert c.run(**over) == inv and c.untouched(), over
    for which, value in (("npts", [2, -1]), ("bo", [0, -16])):
        c = RawCall(M, frames)
        arr = np.array(value, np.int32 if which == "npts" else np.int64)
        assert c.run(**{which: _p(arr)}) == inv and c.untouched(), which
    c = RawCall(M, frames)                                        # info is optional
    assert c.run(info=None) == M.MML_OK and np.all(c.info == -3) and c.kept.tolist() == [2, 300]
    e = RawCall(M, [np.zeros((0, 4), np.float32)])                # no point to read: data may be NULL
    assert e.run(data=None) == M.MML_OK and e.kept.tolist() == [0]
