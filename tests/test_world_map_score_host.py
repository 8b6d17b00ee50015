"""csrc/world_map_score.h on the host: tests/cpp/world_map_score_check.cpp, a program of its own, is built with AddressSanitizer
and UndefinedBehaviorSanitizer where no device is visible (sanitizer builds stay on the CPU machines, as for
tests/cpp/world_map_assoc_check.cpp), runs the header's score arithmetic on scripted and generated cases -- |d| at 0, on both
sides of the gate and exactly at it, a planarity failure, skipped features, strides that leave one and no feature, a pose that is
not a number -- and prints every case with its inputs.  The same inputs go through tests/world_map_score_ref.py and every result
line is compared bit for bit (the results are integers)."""
import os
import shutil
import subprocess

import numpy as np

import world_map_ref as R
import world_map_score_ref as W
from conftest import ROOT


def _f32(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


def _f64(words):
    return np.array([int(w, 16) for w in words], np.uint64).view(np.float64)


def test_score_header_against_the_restatement(has_gpu, tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "world_map_score_check"
    san = [] if has_gpu else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off"] + san +
                         ["-I", os.path.join(ROOT, "multi-modal-loam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "world_map_score_check.cpp"),
                          "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    lines = run.stdout.splitlines()
    assert lines[-1].startswith("S ")
    counts = [int(v) for v in lines[-1].split()[1:]]
    at, cases, seen, looked = 0, 0, [0] * 5, []
    scripted = []
    while lines[at][0] == "C":
        head, Tw, size = [p.split() for p in lines[at][2:].split("|")]
        map, nb, min_points, stride = int(head[0]), int(head[1]), int(head[2]), int(head[6])
        o = dict(neighbourhood=nb, min_points=min_points, min_planarity=_f32(head[3:4])[0], max_plane_dist=float(_f64(head[4:5])[0]), stride=stride)
        inv = _f32(head[5:6])[0]
        T = np.eye(4)
        T[:3] = _f64(Tw).reshape(3, 4)
        nf, nv = int(size[0]), int(size[1])
        f = np.array([_f32(l[2:].split()) for l in lines[at + 1:at + 1 + nf]], np.float32).reshape(-1, 3)
        assert all(l[0] == "F" for l in lines[at + 1:at + 1 + nf])
        table = {}
        for line in lines[at + 1 + nf:at + 1 + nf + nv]:
            assert line[0] == "V"
            ijkn, sw, nw = [p.split() for p in line[2:].split("|")]
            i, j, k, n = (int(v) for v in ijkn)
            sur = np.zeros(8, np.float32)
            sur[:3], sur[6] = _f32(nw[:3]), _f32(nw[3:4])[0]
            table[R.pack(map, i, j, k)] = (_f32(sw) / R.F32(n), n, sur)
        at += 1 + nf + nv
        assert lines[at][0] == "R"
        tot, per = [p.split() for p in lines[at][2:].split("|")]
        tab = W.Table(table, map)
        st, q = W.statuses(tab, inv, f, T[None], o)
        exp = W.score(tab, inv, f, T[None], o)[0]
        assert (int(tot[0]), int(tot[1]), int(tot[2])) == (int(exp["score_q"]), int(exp["n_match"]), int(exp["n_scored"])), (cases, lines[at], exp)
        got_st, got_q = [int(v) for v in per[0::2]], [int(v) for v in per[1::2]]
        assert got_st == st[0].tolist() and got_q == [int(v) for v in q[0]], (cases, lines[at], st, q)
        assert len(got_st) == (0 if nf == 0 else (nf - 1) // stride + 1)
        for s in got_st:
            seen[s] += 1
        looked.append(len(got_st))
        scripted.append((got_st, got_q, stride, nf))
        cases += 1
        at += 1
    assert at == len(lines) - 1 and seen == counts
    # the scripted cases say what they were written for
    st, q, _, _ = scripted[0]
    assert st == [4, 4, 3, 4, 4] and q[0] == 65536 and 0 < q[1] < 100 and q[3] == 0 and q[4] == 0
    assert scripted[1][0] == [2] * 5 and sum(scripted[1][1]) == 0
    assert scripted[2][0][5:] == [0, 0, 1]
    assert [len(s[0]) for s in scripted[3:12]] == [8, 4, 3, 2, 2, 2, 2, 1, 1]
    assert [len(s[0]) for s in scripted[12:16]] == [1, 1, 0, 0]
    assert scripted[16][0] == [0, 0] and scripted[17][0] == [0, 0] and scripted[18][:2] == ([4], [0])
    assert cases >= 300 and min(seen) >= 5 and seen[4] >= 100 and 0 in looked and 1 in looked, (cases, seen)
