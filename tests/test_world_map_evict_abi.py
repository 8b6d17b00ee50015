"""The eviction's C-ABI, what needs no device: include/mmloam_hip.h declares both functions and both structs, the ctypes mirrors
have the sizes and offsets the host C compiler gives the header's structs (compiled as tests/test_abi_structs.py does), the
library exports the symbols, and the refusals decided before a context is touched."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import abi_header as H
from conftest import ROOT

FIELDS = {"mml_wm_evict_rule": ("map", "mode", "lo", "hi", "min_count"), "mml_wm_evict_info": ("n_before", "n_evicted", "n_kept", "first_row")}


def test_header_declares_functions_structs_and_constants(M):
    decls, defines = H.read_header(os.path.join(ROOT, "include", "mmloam_hip.h"))
    assert decls["mml_world_map_evict"] == ("int", ["ptr", "int", "ptr", "unsigned", "ptr", "long"] + ["ptr"] * 6)
    assert decls["mml_wm_index_box"] == ("int", ["float", "ptr", "ptr", "ptr", "ptr"])
    for name in ("mml_world_map_evict", "mml_wm_index_box"):
        res, args = H.ctypes_signature(decls[name])
        assert M.SIGNATURES[name][0] is res and list(M.SIGNATURES[name][1]) == args, name
    assert (defines["MML_WM_EVICT_OUTSIDE"], defines["MML_WM_EVICT_INSIDE"], defines["MML_WM_EVICT_NOBOX"]) == (0, 1, 2)
    assert defines["MML_WM_EVICT_DRY"] == 1 == M.MML_WM_EVICT_DRY
    assert (M.WM_EVICT_OUTSIDE, M.WM_EVICT_INSIDE, M.WM_EVICT_NOBOX) == (0, 1, 2)
    text = H.strip_comments(open(os.path.join(ROOT, "include", "mmloam_hip.h")).read())
    for name in FIELDS:
        assert ("} %s;" % name) in text, name
    # the rule the kernels compile (csrc/world_map_evict.h) is the header's, word for word
    own = H.strip_comments(open(os.path.join(ROOT, "multi-modal-loam_amd", "csrc", "world_map_evict.h")).read())
    body = lambda t: " ".join(t[t.index("#define MML_WM_EVICT_RULE_DEFINED"):t.index("} mml_wm_evict_rule;")].split())
    assert body(own) == body(text)


def test_mirrors_have_the_compilers_layout(M, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    mirrors = {"mml_wm_evict_rule": M.WmEvictRule, "mml_wm_evict_info": M.WmEvictInfo}
    assert all(M.ABI_STRUCTS[k] is v for k, v in mirrors.items())
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mmloam_hip.h"', "int main(void) {"]
    for cname, names in FIELDS.items():
        lines.append('    printf("%s . %%zu 0\\n", sizeof(%s));' % (cname, cname))
        lines += ['    printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, n, cname, n, cname, n) for n in names]
    lines += ["    return 0;", "}", ""]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    out = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    seen = 0
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        cname, field, a, b = line.split()
        m = mirrors[cname]
        if field == ".":
            assert C.sizeof(m) == int(a), line
        else:
            assert [n for n, *_ in m._fields_] == list(FIELDS[cname])
            assert (getattr(m, field).offset, getattr(m, field).size) == (int(a), int(b)), line
        seen += 1
    assert seen == 2 + 5 + 4
    assert C.sizeof(M.WmEvictRule) == 36 and C.sizeof(M.WmEvictInfo) == 4 * C.sizeof(C.c_long)
    r = M.wm_evict_rule(3, M.WM_EVICT_INSIDE, (1, 2, 3), (4, 5, 6), 7)
    assert (r.map, r.mode, list(r.lo), list(r.hi), r.min_count) == (3, 1, [1, 2, 3], [4, 5, 6], 7)


def test_library_exports_the_symbols_and_refuses_a_null_context(M):
    nm = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert {"mml_world_map_evict", "mml_wm_index_box"} <= exported
    L = M.lib()
    rule = (M.WmEvictRule * 1)(M.wm_evict_rule(0))
    assert L.mml_world_map_evict(None, 1, rule, 0, None, 0, None, None, None, None, None, None) == M.MML_ERR_INVALID
    assert hasattr(M.Context, "world_map_evict") and hasattr(M.Context, "world_map_index_box")
    lo, hi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.mml_wm_index_box(0.25, p(np.zeros(3, np.float32)), p(np.ones(3, np.float32)), p(lo), p(hi)) == M.MML_OK
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [5, 5, 5]
