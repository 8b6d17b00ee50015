"""The whole Python-to-C boundary against include/mmloam_hip.h: every declaration of the header has a SIGNATURES entry that the
type rule derives from it, argument for argument; nothing else is in the table but the declared extras; lib() binds exactly the
table; and no call in the package names a function outside it.  Host only: no device is opened."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

import abi_header as H
from conftest import ROOT

PARENT_DECLARATIONS = 174   # mml_* functions the header declared when this test was written: the reader must not lose any
# the library's exports that the public header leaves out, as csrc declares them
NOT_IN_HEADER_DECLS = """
int mml_debug_phase_clocks(const char* family, unsigned long long* out, int capacity, int reset);   /* csrc/capi.hip */
"""


def _header():
    return H.read_header(os.path.join(ROOT, "include", "mmloam_hip.h"))


def test_reader_finds_every_declaration():
    decls, defines = _header()
    assert len(decls) >= PARENT_DECLARATIONS
    assert all(n.startswith("mml_") for n in decls)
    # a few by hand, one per kind of the vocabulary
    assert decls["mml_last_error"] == ("char*", ["ptr"]) and decls["mml_abi_version"] == ("int", [])
    assert decls["mml_destroy"] == ("void", ["ptr"]) and decls["mml_fullwindow_create"] == ("ptr", ["int", "ptr"])
    assert decls["mml_world_map_add"] == ("int", ["ptr", "int", "int", "ptr", "ptr", "unsigned", "ptr"])
    assert decls["mml_world_map_create"] == ("int", ["ptr", "int", "float", "long"])
    assert decls["mml_livox_stream_push"] == ("int", ["ptr", "uint64_t", "ptr", "int"])
    assert decls["mml_copy_bandwidth"] == ("int", ["ptr", "size_t", "int", "ptr"])
    assert decls["mml_debug_fw_replay"][1][7] == "long long" and decls["mml_imu_stream_drop_before"][1] == ["ptr", "double", "long"]
    assert defines["MML_ABI_VERSION"] == 1 and defines["MML_WM_SURFELS"] == 1 and defines["MML_BANK_INCREMENT_BUDGET"] == 1 << 22
    assert defines["MML_TOFS_BATCH_MAX"] == 65535 and defines["MML_MAX_STAGES"] == 32


def test_every_declaration_has_its_entry(M):
    decls, _ = _header()
    for name, decl in decls.items():
        assert name in M.SIGNATURES, "%s is declared in the header and missing from SIGNATURES" % name
        restype, argtypes = M.SIGNATURES[name]
        want_res, want_args = H.ctypes_signature(decl)
        assert restype is want_res, (name, restype, want_res)
        assert len(argtypes) == len(want_args), (name, len(argtypes), len(want_args))
        for k, (got, want) in enumerate(zip(argtypes, want_args)):
            assert got is want, "%s argument %d: %s in the table, %s %s in the header" % (name, k, got.__name__, decl[1][k], want.__name__)


def test_every_entry_is_declared(M):
    decls, _ = _header()
    extra = H.parse_declarations(NOT_IN_HEADER_DECLS)
    assert set(extra) == set(M.NOT_IN_HEADER) and not set(extra) & set(decls)
    assert set(M.SIGNATURES) == set(decls) | set(extra)
    for name, decl in extra.items():
        want_res, want_args = H.ctypes_signature(decl)
        assert M.SIGNATURES[name][0] is want_res and list(M.SIGNATURES[name][1]) == want_args, name


def test_lib_binds_exactly_the_table(M):
    nm = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    L = M.lib()
    bound = [n for n in M.SIGNATURES if n in exported]
    assert len(bound) >= PARENT_DECLARATIONS            # (this tree's library exports all of them)
    for name in bound:
        f = getattr(L, name)
        restype, argtypes = M.SIGNATURES[name]
        assert f.restype is restype, name
        assert len(f.argtypes) == len(argtypes) and all(a is b for a, b in zip(f.argtypes, argtypes)), name


def test_package_calls_only_table_entries(M):
    """Static: every `.mml_<name>` the package's sources reach for is in the table, so no call goes out with ctypes' defaults;
    and nothing but the binder assigns a signature."""
    files = sorted(glob.glob(os.path.join(os.path.dirname(M.__file__), "*.py")))
    assert files
    called = set()
    for path in files:
        src = open(path).read()
        called |= set(re.findall(r"\.(mml_\w+)\b", src))
        assigning = [l for l in src.splitlines() if re.search(r"\.(?:argtypes|restype)\b", l)]      # (the binder's one line)
        assert len(assigning) == (1 if os.path.basename(path) == "__init__.py" else 0), (path, assigning)
    assert len(called) > 100 and called <= set(M.SIGNATURES), sorted(called - set(M.SIGNATURES))


def test_binder_skips_missing_symbols(M):
    class F:
        restype, argtypes = "unset", "unset"

    class Stub:      # a library that lacks two of the table's names, as an older build loaded through $MML_LIB_PATH would
        pass
    names = list(M.SIGNATURES)
    missing = {names[3], names[-1]}
    stub = Stub()
    for n in names:
        if n not in missing:
            setattr(stub, n, F())
    M._bind(stub)
    for n in names:
        if n in missing:
            assert not hasattr(stub, n)
        else:
            assert getattr(stub, n).restype is M.SIGNATURES[n][0] and getattr(stub, n).argtypes is M.SIGNATURES[n][1], n


def test_argtypes_refuse_what_the_defaults_let_through(M):
    """What the table is for: a scalar of the wrong width and a float for an int are refused at the call, on the host."""
    L = M.lib()
    with pytest.raises(C.ArgumentError):
        L.mml_marginalize_dense(None, C.c_int(1), None, None, None, None)      # int for long
    with pytest.raises(C.ArgumentError):
        L.mml_world_map_reset(None, 0.5)
    assert L.mml_world_map_reset(None, -1) == M.MML_ERR_INVALID
