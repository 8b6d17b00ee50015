"""The host side of mml_scan_upload_wire_batch: the record layouts of csrc/wire_decode.h (mml_wire_decode_host) against a numpy
restatement, the argument rules (mml_scan_upload_wire_plan), and the header compiled stand-alone under sanitizers.  No device."""
import os
import re
import subprocess

import numpy as np
import pytest

import wire_cases as W
from conftest import ROOT

INVALID, CAPACITY = -1, -4
# point_step -> field offsets (x, y, z, intensity): in order, shuffled, at every alignment mod 4, without an intensity field
LAYOUTS = [(12, (8, 0, 4, -1)), (16, (12, 4, 0, 8)), (19, (1, 6, 11, 15)), (22, (0, 4, 8, 12)), (22, (18, 2, 13, 7)), (23, (19, 3, 9, 14)),
           (32, (0, 4, 8, 16)), (32, (5, 26, 11, 18)), (255, (251, 0, 127, 66)), (256, (252, 129, 2, 67)), (22, (0, 4, 8, -1))]
NINE = ([5, 0, 17, 300, 0, 1, 64, 0, 33], [300, 7, 0, 0, 0, 256, 1, 19, 2])   # empty frames (4), a frame with one empty part


def test_symbols_and_abi(M):
    header = open(M.HEADER_PATH).read()
    for name in ("mml_scan_upload_wire_batch", "mml_scan_upload_wire_plan", "mml_wire_decode_host"):
        assert hasattr(M.lib(), name) and re.search(r"\b%s\(" % name, header), name
    # the version is the header's: additions to the C-ABI have left it at 1 (tests/test_registered_cloud.py, __graft_entry__.build)
    assert re.search(r"#define\s+MML_ABI_VERSION\s+1\b", header) and M.lib().mml_abi_version() == 1


def _check(M, call):
    v, l = M.wire_decode_host(*call["args"])
    assert np.array_equal(W.words(v) if len(v) else np.zeros((0, 4), np.uint32), np.concatenate(call["velo"]))
    assert np.array_equal(W.words(l) if len(l) else np.zeros((0, 5), np.uint32), np.concatenate(call["livox"]))
    return v, l


@pytest.mark.parametrize("step,offs", LAYOUTS)
@pytest.mark.parametrize("rec_bytes", [19, 20])
def test_decode_matches_numpy(M, step, offs, rec_bytes):
    rng = np.random.default_rng(step * 100 + rec_bytes)
    for residue in range(4):   # with nine frames every frame start meets every residue
        call = _check(M, W.make_call(rng, NINE[0], NINE[1], step, offs, rec_bytes, first_residue=residue))
    v, l = call
    assert len(v) == sum(NINE[0]) and len(l) == sum(NINE[1])
    one = W.make_call(rng, [257], [300], step, offs, rec_bytes, first_residue=3)    # count = 1
    v, l = _check(M, one)
    for f in ("reflectivity", "tag", "line"):
        assert set(l[f].tolist()) == set(range(256))
    assert (l["_pad"] == 0).all() if rec_bytes == 19 else len(set(l["_pad"].tolist())) > 100
    k = len(W.SPECIAL)
    got = W.words(v)[:k]
    for j, o in enumerate(offs):    # NaN payloads, signalling NaNs, -0, denormals, infinities: the very words
        assert np.array_equal(got[:, j], np.roll(W.SPECIAL, j) if o >= 0 else np.zeros(k, np.uint32))
    assert np.array_equal(W.words(l)[:k, 1], W.SPECIAL)


def test_gaps_are_not_read(M):
    rng = np.random.default_rng(3)
    call = W.make_call(rng, [3, 2, 4], [2, 5, 1], 22, (0, 4, 8, 12), 19, first_residue=1)
    vd, va, nv = call["args"][0], call["args"][1], call["args"][2]
    assert va[0] > 0 and (vd[:va[0]] == 0xA5).all() and va[1] > va[0] + 22 * nv[0] and (vd[va[0] + 22 * nv[0]:va[1]] == 0xA5).all()
    v0, l0 = M.wire_decode_host(*call["args"])
    keep = np.zeros(len(vd), bool)
    for a, k in zip(va, nv):
        keep[a:a + 22 * k] = True
    vd2 = np.where(keep, vd, 0x11).astype(np.uint8)   # other bytes in the gaps: the same points
    v1, _ = M.wire_decode_host(vd2, *call["args"][1:])
    assert v0.tobytes() == v1.tobytes()


def test_absent_sensor_and_empty_call(M):
    rng = np.random.default_rng(4)
    call = W.make_call(rng, [0, 0, 0], [7, 0, 9], 32, (0, 4, 8, 12), 19)
    assert call["args"][0] is None
    a = list(call["args"])
    a[1] = None   # no offsets either
    v, l = M.wire_decode_host(*a)
    assert len(v) == 0 and np.array_equal(W.words(l), np.concatenate(call["livox"]))
    call = W.make_call(rng, [4, 0, 2], [0, 0, 0], 32, (0, 4, 8, 12), 20)
    v, l = _check(M, call)
    assert len(l) == 0 and len(v) == 6
    rc, span, bad = M.scan_upload_wire_plan(None, [0, 0], 22, (0, 4, 8, 12), None, [0, 0])
    assert rc == 0 and bad == -1 and not span.any()
    a = list(W.make_call(rng, [4], [1], 22, (0, 4, 8, 12), 19)["args"])
    a[0] = None   # points announced, no bytes
    with pytest.raises(M.MmlError):
        M.wire_decode_host(*a)


def _plan(M, va, nv, la, nl, step=22, offs=(0, 4, 8, 12), rec=19, **caps):
    return M.scan_upload_wire_plan(va, nv, step, offs, la, nl, rec, **caps)


def test_plan_span(M):
    rng = np.random.default_rng(5)
    call = W.make_call(rng, NINE[0], NINE[1], 23, (19, 3, 9, 14), 19, first_residue=2)
    vd, va, nv, _, _, ld, la, nl, _ = call["args"]
    rc, span, bad = _plan(M, va, nv, la, nl, step=23, offs=(19, 3, 9, 14))
    assert rc == 0 and bad == -1
    # first payload's first byte .. one past the last payload's last byte (the buffers end there); the gap in front stays out
    assert span.tolist() == [int(va[0]), len(vd), int(la[0]), len(ld)] and va[0] > 0 and la[0] > 0
    # leading and trailing empty frames do not widen the span
    rc, span, _ = _plan(M, [0, 40, 40 + 44, 500], [0, 2, 1, 0], [3, 3, 3, 3], [0, 0, 0, 0])
    assert rc == 0 and span.tolist() == [40, 40 + 44 + 22, 0, 0]


def test_plan_refusals(M):
    va, nv, la, nl = [0, 100, 200], [4, 4, 4], [0, 100, 200], [5, 5, 5]
    assert _plan(M, va, nv, la, nl)[0] == 0
    assert _plan(M, [0, 88, 176], nv, [0, 95, 190], nl)[0] == 0                      # payloads that touch
    for bad_args, frame in (((([0, 200, 100]), nv, la, nl), 2),                     # decreasing offsets
                            ((va, nv, [0, 100, 99], nl), 2),
                            (([0, 87, 200], nv, la, nl), 1),                         # overlap by one byte
                            ((va, nv, [0, 94, 200], nl), 1),
                            ((va, [4, -1, 4], la, nl), 1),                           # negative counts
                            ((va, nv, la, [5, 5, -3]), 2),
                            (([-1, 100, 200], nv, la, nl), 0)):                      # negative offset
        rc, span, bad = _plan(M, *bad_args)
        assert rc == INVALID and bad == frame and not span.any(), (bad_args, rc, bad)
    # an empty frame's offset counts too
    assert _plan(M, [0, 50, 200], [4, 0, 4], la, nl)[::2] == (INVALID, 1)
    for kw in (dict(offs=(0, 4, 8, 19)), dict(offs=(0, 4, 19, 12)), dict(offs=(-1, 4, 8, 12)), dict(step=11, offs=(0, 4, 7, -1)),
               dict(step=257), dict(rec=18), dict(rec=21)):
        rc, span, bad = _plan(M, va, nv, la, nl, **kw)
        assert rc == INVALID and bad == -1, kw
    assert _plan(M, va, nv, la, nl, step=12, offs=(0, 4, 8, -1))[0] == 0
    assert _plan(M, [0, 1024, 2048], nv, la, nl, step=256, offs=(0, 4, 8, 252))[0] == 0
    assert _plan(M, [0] * 3, [0] * 3, la, nl, rec=20)[0] == 0
    # capacities: exactly at capacity passes, one over names its frame
    va, la = np.arange(8) * 100000, np.arange(8) * 100000
    nv, nl = [512, 0, 511, 512, 1, 512, 512, 512], [512] * 8
    assert _plan(M, va, nv, la, nl, max_velo_points=512, max_livox_points=512)[0] == 0
    nv[6] = 513
    assert _plan(M, va, nv, la, nl, max_velo_points=512, max_livox_points=512)[::2] == (CAPACITY, 6)
    assert _plan(M, va, nv, la, nl, max_velo_points=513, max_livox_points=512)[0] == 0
    nl[5] = 513
    assert _plan(M, va, nv, la, nl, max_velo_points=513, max_livox_points=512)[::2] == (CAPACITY, 5)
    assert _plan(M, va, nv, la, nl)[0] == 0                                          # no capacity given: not checked
    assert M.scan_upload_wire_plan([], [], 22, (0, 4, 8, 12), [], [])[0] == INVALID  # count 0


def _case_bytes(args, caps=(-1, -1)):
    vd, va, nv, step, offs, ld, la, nl, rec = args
    vd = np.zeros(0, np.uint8) if vd is None else vd
    ld = np.zeros(0, np.uint8) if ld is None else ld
    head = np.array([len(nv), step, *offs, rec, *caps], "<i4").tobytes() + np.array([len(vd), len(ld)], "<i8").tobytes()
    return head + np.asarray(va, "<i8").tobytes() + np.asarray(nv, "<i4").tobytes() + np.asarray(la, "<i8").tobytes() + \
        np.asarray(nl, "<i4").tobytes() + vd.tobytes() + ld.tobytes()


def test_header_under_sanitizers(M, tmp_path):
    """csrc/wire_decode.h compiled by the host compiler into a stand-alone program with AddressSanitizer and
    UndefinedBehaviorSanitizer.  Its buffers are exactly as long as the data and every case's last payload ends on the buffer's
    last byte: a decode that read a rounded-up word behind the span would be reported.  Its words must equal the library's."""
    exe = tmp_path / "wire_decode_replay"
    csrc = os.path.join(os.path.dirname(M.LIB_PATH), "csrc")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "cpp", "wire_decode_replay.cpp"),
                          "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    rng = np.random.default_rng(9)
    calls = []
    for (step, offs), rec in zip(LAYOUTS, [19, 20] * 6):
        for residue in range(4):
            calls.append(W.make_call(rng, NINE[0], NINE[1], step, offs, rec, first_residue=residue, lead=residue & 1 == 0))
    calls.append(W.make_call(rng, [1], [1], 12, (8, 0, 4, -1), 19, lead=False, gaps=False))   # the buffer IS the record
    calls.append(W.make_call(rng, [0, 0], [0, 3], 256, (252, 129, 2, 67), 19))
    for c in calls:   # every call ends on its buffers' last bytes
        vd, va, nv, step, _, ld, la, nl, rec = c["args"]
        assert vd is None or max(a + k * step for a, k in zip(va, nv) if k) == len(vd)
        assert ld is None or max(a + k * rec for a, k in zip(la, nl) if k) == len(ld)
    refused = [(([0, 87], [4, 4], 22, (0, 4, 8, 12), [0, 0], [0, 0], 19), (-1, -1), (INVALID, 1)),
               (([0, 100], [4, 5], 22, (0, 4, 8, 12), [0, 0], [0, 0], 19), (4, 4), (CAPACITY, 1))]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(calls) + len(refused)], "<i4").tobytes())
        for c in calls:
            f.write(_case_bytes(c["args"]))
        for (va, nv, step, offs, la, nl, rec), caps, _ in refused:
            f.write(_case_bytes((None, va, nv, step, offs, None, la, nl, rec), caps))
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]
    lines = run.stdout.split("\n")
    for c in calls:
        a = c["args"]
        rc, span, bad = M.scan_upload_wire_plan(a[1], a[2], a[3], a[4], a[6], a[7], a[8])
        assert [int(x) for x in lines.pop(0).split()] == [rc, bad] + span.tolist() and rc == 0
        v, l = M.wire_decode_host(*a)
        for got, want in ((lines.pop(0), v), (lines.pop(0), l)):
            got = np.array([int(x, 16) for x in got.split()], np.uint32)
            assert np.array_equal(got, W.words(want).reshape(-1) if len(want) else np.zeros(0, np.uint32))
    for _, _, (rc, bad) in refused:
        assert [int(x) for x in lines.pop(0).split()][:2] == [rc, bad]
    assert lines == [""]


def build_adapter_probe(out_path):
    """tests/cpp/wire_batch_probe.cpp (feature_extraction::unionCloudWire of host/mmloam_adapter.hpp) against the built library."""
    libdir = os.path.join(ROOT, "multi-modal-loam_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(libdir, "host"),
           os.path.join(ROOT, "tests", "cpp", "wire_batch_probe.cpp"), "-o", str(out_path), "-L", libdir, "-lmmloam_hip",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_adapter_probe_compiles_and_links(tmp_path):
    build_adapter_probe(tmp_path / "wire_batch_probe")
