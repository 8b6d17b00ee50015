"""Every ctypes.Structure and numpy dtype that mirrors a struct of include/mmloam_hip.h (ABI_STRUCTS) against the C compiler's
own layout: one host program, generated from the mapping, prints sizeof and each named field's offsetof and size.  Host only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NOT_HEADER_STRUCTS = {"POINTXYZINORMAL_DTYPE"}     # pcl::PointXYZINormal: a record of PCL's, not of the header


def _mirrors(M):
    """[(C struct name, mirror's name, size, {field: (offset, size)})] for every mirror of ABI_STRUCTS"""
    out = []
    for cname, mirror in M.ABI_STRUCTS.items():
        for m in mirror if isinstance(mirror, tuple) else (mirror,):
            if isinstance(m, np.dtype):
                out.append((cname, str(m.names), m.itemsize, {n: (m.fields[n][1], m.fields[n][0].itemsize) for n in m.names}))
            else:
                assert issubclass(m, C.Structure), cname
                out.append((cname, m.__name__, C.sizeof(m), {n: (getattr(m, n).offset, getattr(m, n).size) for n, *_ in m._fields_}))
    return out


@pytest.fixture(scope="module")
def c_layout(M, tmp_path_factory):
    """{C struct name: (sizeof, {field: (offsetof, sizeof)})} as the host C compiler lays the header's structs out"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    fields = {}
    for cname, _, _, f in _mirrors(M):
        fields.setdefault(cname, []).extend(n for n in f if n not in fields.get(cname, []))
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "mmloam_hip.h"', "int main(void) {"]
    for cname, names in fields.items():
        lines.append('    printf("%s . %%zu 0\\n", sizeof(%s));' % (cname, cname))
        lines += ['    printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, n, cname, n, cname, n) for n in names]
    lines += ["    return 0;", "}", ""]
    d = tmp_path_factory.mktemp("abi_structs")
    src, exe = d / "layout.c", d / "layout"
    src.write_text("\n".join(lines))
    out = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, check=True)
    layout = {}
    for line in run.stdout.splitlines():
        cname, field, a, b = line.split()
        if field == ".":
            layout[cname] = (int(a), {})
        else:
            layout[cname][1][field] = (int(a), int(b))
    return layout


def test_mapping_covers_every_mirror(M):
    mapped = [m for v in M.ABI_STRUCTS.values() for m in (v if isinstance(v, tuple) else (v,))]
    for name, obj in vars(M).items():
        if isinstance(obj, type) and issubclass(obj, C.Structure) and obj is not C.Structure:
            assert any(obj is m for m in mapped), "ctypes.Structure %s is in no entry of ABI_STRUCTS" % name
        if isinstance(obj, np.dtype) and obj.names and name not in NOT_HEADER_STRUCTS:
            assert any(obj is m for m in mapped), "dtype %s is in no entry of ABI_STRUCTS" % name
    assert len(mapped) >= 25 + 7 and all(k.startswith("mml_") for k in M.ABI_STRUCTS)


def test_sizes_and_field_offsets(M, c_layout):
    assert set(c_layout) == set(M.ABI_STRUCTS)
    for cname, pyname, size, fields in _mirrors(M):
        c_size, c_fields = c_layout[cname]
        assert size == c_size, "%s: %s is %d bytes, the C struct %d" % (cname, pyname, size, c_size)
        for n, (off, sz) in fields.items():
            assert (off, sz) == c_fields[n], "%s.%s: offset, size %s in %s, %s in C" % (cname, n, (off, sz), pyname, c_fields[n])
        # the fields tile the struct up to alignment padding: the last one ends within 8 bytes of the end
        assert c_size - max(o + s for o, s in fields.values()) < 8, cname
