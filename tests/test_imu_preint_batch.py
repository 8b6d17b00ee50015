"""mml_imu_preintegrate_batch with a NULL context -- the host build of csrc/imu_preint.h, the routine the device runs -- against
mml_imu_preintegrate (bytes wherever no sin / cos of a step angle is taken; elsewhere the bytes of dp, dv, dq, dtime, bg, ba and
the tolerances of tests/test_imu.py on the rest) and against oracle/imu_oracle.py::preintegrate; the argument checks; odometry.preintegrate_windows; the adapter's
PreIntegrationBatch.  The input builders are shared with tests/test_gpu_imu_preint_batch.py."""
import ctypes as C
import importlib
import os
import re
import subprocess
import textwrap

import numpy as np
import pytest

import imu_oracle as IO
from conftest import ROOT

BG, BA = np.array([0.01, -0.02, 0.005]), np.array([0.05, 0.02, -0.03])
GATE = 0.00001  # IMUIntegrator.cpp:129: the right Jacobian is the identity up to this step angle


def family(rng, n, dt_lo=0.004, dt_hi=0.006, gyro=0.0):
    """The family of tests/test_imu.py: gyro N(gyro, 0.3), accel N((0, 0, 1), 0.2) in message units, dt uniform."""
    return np.concatenate([rng.normal(0, 0.3, (n, 3)) + gyro, rng.normal(0, 0.2, (n, 3)) + [0, 0, 1.0],
                           rng.uniform(dt_lo, dt_hi, (n, 1))], axis=1)


def still(rng, n, bg):
    """Gyro exactly equal to bg: every step angle is exactly 0."""
    s = family(rng, n)
    s[:, :3] = bg
    return s


def gated(rng, n, below):
    """Zero gyro bias, every sample turning about x by exactly GATE (`below`: by the double before it): the comparison
    nrm > 0.00001 is false for both, so no sin / cos of nrm is taken."""
    s = family(rng, n)
    dt = 2.0 ** -8                                # a power of two: x * dt is exact
    x = (np.nextafter(GATE, 0.0) if below else GATE) / dt
    s[:, 0], s[:, 1:3], s[:, 6] = x, 0.0, dt
    return s


def large_rotation(rng):
    """40 samples of 5 ms at about 18 rad/s: 3.6 rad in all, through 180 degrees.  Past 120 degrees the trace of
    dq.matrix() dR is negative (m3_to_quat's second branch); past 180 that branch, which makes the largest component (z,
    positive here) positive, returns w < 0 and the sign is flipped."""
    return family(rng, 40, 0.005, 0.005, gyro=np.array([10.5, -8.0, 12.3]))


def tolerance_cases(synth):
    """(name, samples, bg, ba) of the comparison against the oracle and the single call."""
    rng = np.random.default_rng(1)
    return [("test_imu family", family(rng, 40), BG, BA),
            ("synth.imu_samples", synth.imu_samples(20, 21), np.zeros(3), np.zeros(3)),
            ("200 samples at 0.5 ms", family(rng, 200, 0.0005, 0.0005), BG, BA),
            ("large rotation", large_rotation(rng), BG, BA)]


def byte_cases():
    """(name, samples, bg, ba): no step angle above the gate, so the single call takes no libm sin / cos."""
    rng = np.random.default_rng(2)
    z = np.zeros(3)
    out = [("empty", np.zeros((0, 7)), BG, BA)]
    for n in (1, 2, 65):
        out.append(("gyro == bg, %d" % n, still(rng, n, BG), BG, BA))
        out.append(("at the gate, %d" % n, gated(rng, n, False), z, BA))
        out.append(("below the gate, %d" % n, gated(rng, n, True), z, BA))
    return out


def mixed_batch(synth):
    """Different lengths, a bias pair per interval, empty intervals between, in one shared samples array."""
    rng = np.random.default_rng(3)
    smp = [family(rng, 7), np.zeros((0, 7)), synth.imu_samples(30, 31), large_rotation(rng), np.zeros((0, 7)), family(rng, 1),
           family(rng, 33), still(rng, 2, BG), family(rng, 64, 0.001, 0.003), np.zeros((0, 7))]
    n = len(smp)
    bg = rng.normal(0, 0.01, (n, 3))
    ba = rng.normal(0, 0.03, (n, 3))
    bg[7] = BG
    return smp, bg, ba


def ratios(pre, ref_R, ref):
    """Worst error over tolerance per field, with the tolerances tests/test_imu.py holds the single call to."""
    from scipy.spatial.transform import Rotation as Rsc
    r = {}
    r["dp"] = np.abs(np.array(pre.dp) - ref["dp"]).max() / 1e-12
    r["dv"] = np.abs(np.array(pre.dv) - ref["dv"]).max() / 1e-12
    r["dR"] = np.abs(Rsc.from_quat(np.array(pre.dq)).as_matrix() - ref_R).max() / 1e-12
    J, Jr = np.array(pre.jacobian).reshape(15, 15), ref["jacobian"]
    r["jacobian"] = (np.abs(J - Jr) / (1e-13 + 1e-10 * np.abs(Jr))).max()
    P, Pr = np.array(pre.covariance).reshape(15, 15), ref["covariance"]
    r["covariance"] = (np.abs(P - Pr) / (1e-20 + 1e-10 * np.abs(Pr))).max()
    return r


def as_ref(pre):
    from scipy.spatial.transform import Rotation as Rsc
    return dict(dp=np.array(pre.dp), dv=np.array(pre.dv), dR=Rsc.from_quat(np.array(pre.dq)).as_matrix(),
                jacobian=np.array(pre.jacobian).reshape(15, 15), covariance=np.array(pre.covariance).reshape(15, 15))


def test_header_declares_and_library_exports_the_symbol(M):
    header = open(M.HEADER_PATH).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", M.LIB_PATH], text=True)
    assert re.search(r"\bint\s+mml_imu_preintegrate_batch\s*\(\s*mml_ctx\s*\*\s*ctx\s*,", header)
    assert re.search(r"#define\s+MML_PREINT_BATCH_MAX\s+%d\b" % M.PREINT_BATCH_MAX, header) and M.PREINT_BATCH_MAX == 8192
    assert re.search(r"\bT mml_imu_preintegrate_batch$", syms, re.M)
    assert re.search(r"#define\s+MML_ABI_VERSION\s+1\b", header) and M.lib().mml_abi_version() == 1
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    assert callable(M.imu_preintegrate_batch) and callable(odometry.preintegrate_windows)


def test_bytes_of_the_single_call_where_no_sin_or_cos_is_taken(M):
    cases = byte_cases()
    assert len(cases) == 10
    for name, s, bg, ba in cases:
        (pre,) = M.imu_preintegrate_batch([s], bg, ba)
        assert bytes(pre) == bytes(M.imu_preintegrate(s, bg, ba)), name
        if len(s):
            gdt = (s[:, :3] - bg) * s[:, 6:7]
            nrm = np.sqrt((gdt[:, 0] * gdt[:, 0] + gdt[:, 1] * gdt[:, 1]) + gdt[:, 2] * gdt[:, 2])
            want = GATE if name.startswith("at") else np.nextafter(GATE, 0.0) if name.startswith("below") else 0.0
            assert np.all(nrm == want), name
    (pre,) = M.imu_preintegrate_batch([np.zeros((0, 7))], BG, BA)          # the reset state
    assert np.array_equal(np.array(pre.jacobian).reshape(15, 15), np.eye(15)) and not np.any(np.array(pre.covariance))
    assert list(pre.dq) == [0, 0, 0, 1] and pre.dtime == 0 and not np.any(list(pre.dp) + list(pre.dv))
    assert np.array_equal(np.array(pre.bg), BG) and np.array_equal(np.array(pre.ba), BA)


def test_state_bytes_of_the_single_call_where_sin_and_cos_are_taken(M, synth):
    """Every step rotates by more than the gate, so the single call takes libm's sin / cos and the batch call mml_sin / mml_cos
    -- in the right Jacobian only, which feeds the Jacobian and covariance chains and nothing else: dp, dv, dq, dtime, bg, ba
    (the struct up to `jacobian`) have the single call's bytes.  The two calls run one routine (csrc/imu_preint.h) that differs
    in that choice alone; a choice wired to any other sin / cos (so3_exp's) would show here."""
    state = M.ImuPreint.jacobian.offset
    assert state == 17 * 8 and M.ImuPreint.covariance.offset == state + 225 * 8
    cases = tolerance_cases(synth)
    smp, bgs, bas = mixed_batch(synth)
    cases += [("mixed %d" % i, s, bgs[i], bas[i]) for i, s in enumerate(smp) if i in (0, 2, 3, 6, 8)]
    assert len(cases) == 9
    for name, s, bg, ba in cases:
        gdt = (s[:, :3] - bg) * s[:, 6:7]
        nrm = np.sqrt((gdt[:, 0] * gdt[:, 0] + gdt[:, 1] * gdt[:, 1]) + gdt[:, 2] * gdt[:, 2])
        assert len(s) and np.all(nrm > GATE), name
        (pre,) = M.imu_preintegrate_batch([s], bg, ba)
        assert bytes(pre)[:state] == bytes(M.imu_preintegrate(s, bg, ba))[:state], name


def test_against_the_oracle_and_the_single_call(M, synth):
    """dp, dv, rotation atol 1e-12; Jacobian rtol 1e-10, atol 1e-13; covariance rtol 1e-10, atol 1e-20 (tests/test_imu.py).
    Prints the worst error / tolerance ratios (DESIGN_8F.md records them)."""
    for name, s, bg, ba in tolerance_cases(synth):
        (pre,) = M.imu_preintegrate_batch([s], bg, ba)
        ref = IO.preintegrate(s, bg, ba)
        one = as_ref(M.imu_preintegrate(s, bg, ba))
        gdt = (s[:, :3] - bg) * s[:, 6:7]
        assert np.linalg.norm(gdt, axis=1).max() > GATE, name             # the mml_sin / mml_cos path is taken
        if name == "large rotation":
            assert np.trace(ref["dR"]) < 0 and np.linalg.norm(gdt, axis=1).sum() > np.pi
        for what, r, dR in (("oracle", ref, ref["dR"]), ("single call", one, one["dR"])):
            q = ratios(pre, dR, r)
            print("%-24s vs %-12s %s" % (name, what, "  ".join("%s %.3g" % kv for kv in q.items())))
            assert np.allclose(np.array(pre.dp), r["dp"], rtol=0, atol=1e-12), (name, what)
            assert np.allclose(np.array(pre.dv), r["dv"], rtol=0, atol=1e-12), (name, what)
            assert np.allclose(as_ref(pre)["dR"], dR, rtol=0, atol=1e-12), (name, what)
            assert np.allclose(np.array(pre.jacobian).reshape(15, 15), r["jacobian"], rtol=1e-10, atol=1e-13), (name, what)
            assert np.allclose(np.array(pre.covariance).reshape(15, 15), r["covariance"], rtol=1e-10, atol=1e-20), (name, what)
        assert abs(pre.dtime - ref["dtime"]) < 1e-15 * max(1, len(s)) and pre.dq[3] >= 0
        assert abs(np.linalg.norm(np.array(pre.dq)) - 1.0) < 1e-15


def test_mixed_batch_equals_single_interval_calls(M, synth):
    smp, bg, ba = mixed_batch(synth)
    out = M.imu_preintegrate_batch(smp, bg, ba)
    assert len(out) == len(smp) == 10
    for i, s in enumerate(smp):
        (one,) = M.imu_preintegrate_batch([s], bg[i], ba[i])
        assert bytes(out[i]) == bytes(one), i
    assert len({bytes(p) for p in out}) == 10
    same = M.imu_preintegrate_batch(smp[:3], BG, BA)                       # one bias pair for all
    each = M.imu_preintegrate_batch(smp[:3], np.tile(BG, (3, 1)), np.tile(BA, (3, 1)))
    assert [bytes(p) for p in same] == [bytes(p) for p in each]
    with pytest.raises(ValueError):
        M.imu_preintegrate_batch(smp[:3], np.zeros((2, 3)), BA)


def refusals(M):
    """(name, n, samples, offsets, bg, ba, out is null) of every MML_ERR_INVALID case; arrays sized for 3 intervals."""
    s, b = np.zeros((6, 7)), np.zeros((3, 3))
    ok = np.array([0, 2, 2, 6], np.int32)
    big = np.zeros(M.PREINT_BATCH_MAX + 2, np.int32)
    return [("n = 0", 0, s, ok, b, b, False), ("n < 0", -1, s, ok, b, b, False),
            ("n too large", M.PREINT_BATCH_MAX + 1, s, big, b, b, False),
            ("null samples", 3, None, ok, b, b, False), ("null offsets", 3, s, None, b, b, False),
            ("null bg", 3, s, ok, None, b, False), ("null ba", 3, s, ok, b, None, False), ("null out", 3, s, ok, b, b, True),
            ("offsets[0] != 0", 3, s, np.array([1, 2, 2, 6], np.int32), b, b, False),
            ("decreasing offset", 3, s, np.array([0, 4, 3, 6], np.int32), b, b, False)]


def check_refusals(M, ctx):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for name, n, s, off, bg, ba, null_out in refusals(M):
        out = (M.ImuPreint * 3)()
        C.memset(out, 0xAB, C.sizeof(out))
        before = bytes(out)
        rc = M.lib().mml_imu_preintegrate_batch(ctx._h if ctx is not None else None, n, p(s), p(off), p(bg), p(ba), None if null_out else out)
        assert rc == M.MML_ERR_INVALID, name
        assert bytes(out) == before, name
        if ctx is not None:
            msg = M.lib().mml_last_error(ctx._h).decode()
            assert "mml_imu_preintegrate_batch" in msg, (name, msg)
            if name == "decreasing offset":
                assert "interval 1" in msg, msg


def test_invalid_arguments_leave_the_output_untouched(M):
    check_refusals(M, None)
    with pytest.raises(M.MmlError) as e:
        M.imu_preintegrate_batch([], BG, BA)
    assert e.value.code == M.MML_ERR_INVALID
    out = (M.ImuPreint * 1)()                                               # no samples at all: samples may be null
    z, off = np.zeros((1, 3)), np.zeros(2, np.int32)
    assert M.lib().mml_imu_preintegrate_batch(None, 1, None, off.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p),
                                              z.ctypes.data_as(C.c_void_p), out) == M.MML_OK
    assert bytes(out[0]) == bytes(M.imu_preintegrate(np.zeros((0, 7)), z[0], z[0]))


def windows(synth, n=2, W=3, k0=20, seed=4):
    """samples[w][f], frames[w][f] (bg / ba only) for preintegrate_windows: synth.imu_samples between consecutive scans."""
    rng = np.random.default_rng(seed)
    samples = [[None] + [synth.imu_samples(k0 + W * w + f - 1, k0 + W * w + f) for f in range(1, W)] for w in range(n)]
    frames = [[dict(bg=rng.normal(0, 1e-3, 3), ba=rng.normal(0, 1e-2, 3)) for _ in range(W)] for _ in range(n)]
    return samples, frames


def test_preintegrate_windows_returns_what_per_interval_calls_return(M, synth):
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    samples, frames = windows(synth)
    samples.append([None])                                                  # a window of one frame has no interval
    frames.append([dict(bg=np.zeros(3), ba=np.zeros(3))])
    pres = odometry.preintegrate_windows(samples, frames)
    assert [len(p) for p in pres] == [3, 3, 1] and all(p[0] is None for p in pres)
    for w in range(2):
        for f in (1, 2):
            (one,) = M.imu_preintegrate_batch([samples[w][f]], frames[w][f - 1]["bg"], frames[w][f - 1]["ba"])
            assert bytes(pres[w][f]) == bytes(one), (w, f)
    assert odometry.preintegrate_windows([], []) == []
    with pytest.raises(ValueError):
        odometry.preintegrate_windows(samples[:2], frames)
    with pytest.raises(ValueError):
        odometry.preintegrate_windows([samples[0][:2]], frames[:1])


def test_cpp_adapter_preintegration_batch(M, tmp_path):
    """mml::IMUIntegrator::PreIntegrationBatch (host/mmloam_adapter.hpp) with a null context against the Python call."""
    rng = np.random.default_rng(5)
    smp = [family(rng, 5), family(rng, 0), family(rng, 34)]
    src = tmp_path / "preint_probe.cpp"
    src.write_text(textwrap.dedent(r"""
        #include <cstdio>
        #include <vector>
        #include "mmloam_adapter.hpp"
        int main(int argc, char** argv) {
            FILE* f = std::fopen(argv[1], "r");
            std::vector<mml::IMUIntegrator> imu(3);
            std::vector<mml::Vector3d> bg(3), ba(3);
            for (int i = 0; i < 3; ++i) {
                int n = 0;
                if (std::fscanf(f, "%d %lf %lf %lf %lf %lf %lf", &n, &bg[i].v[0], &bg[i].v[1], &bg[i].v[2], &ba[i].v[0], &ba[i].v[1],
                                &ba[i].v[2]) != 7) return 2;
                for (int k = 0; k < n; ++k) {
                    double m[7];
                    for (int j = 0; j < 7; ++j) if (std::fscanf(f, "%lf", &m[j]) != 1) return 3;
                    imu[i].PushIMUMsg(m);
                }
            }
            std::vector<mml::IMUIntegrator*> p = {&imu[0], &imu[1], &imu[2]};
            std::vector<mml_imu_preint> out;
            mml::IMUIntegrator::PreIntegrationBatch(nullptr, p, bg, ba, &out);
            for (int i = 0; i < 3; ++i) {
                if (!imu[i].has_pre || imu[i].dq.w != out[i].dq[3]) return 4;
                const double* d = reinterpret_cast<const double*>(&imu[i].pre);
                for (size_t k = 0; k < sizeof(mml_imu_preint) / sizeof(double); ++k) std::printf("%.17g ", d[k]);
                std::printf("\n");
            }
            return 0;
        }"""))
    bg, ba = rng.normal(0, 0.01, (3, 3)), rng.normal(0, 0.03, (3, 3))
    data = tmp_path / "imu.txt"
    with open(data, "w") as f:
        for i, s in enumerate(smp):
            f.write("%d %s %s\n" % (len(s), " ".join("%.17g" % v for v in bg[i]), " ".join("%.17g" % v for v in ba[i])))
            for row in s:
                f.write(" ".join("%.17g" % v for v in row) + "\n")
    exe = tmp_path / "preint_probe"
    libdir = os.path.join(ROOT, "multi-modal-loam_amd")
    cmd = ["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"), str(src), "-o", str(exe),
           "-L", libdir, "-lmmloam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    ref = M.imu_preintegrate_batch(smp, bg, ba)
    for line, r in zip(run.stdout.strip().split("\n"), ref):
        assert np.array_equal(np.array([float(v) for v in line.split()]), np.frombuffer(bytes(r), dtype=np.float64))
