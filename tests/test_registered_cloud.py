"""CPU suite for the registered-cloud output (mml_cloud_download_registered / _batch): the C-ABI surface and the argument
checks of the Python wrapper.  The device side is tests/test_gpu_registered_cloud.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("mml_cloud_download_registered", "mml_cloud_download_registered_batch")


def test_declared_in_the_header_and_exported(M):
    src = open(os.path.join(ROOT, "include", "mmloam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = re.findall(r"\bint\s+(mml_[a-z0-9_]+)\s*\(", src)
    nm = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NAMES:
        assert declared.count(name) == 1, name
        assert name in exported, name


def test_abi_version_is_still_1(M):
    src = open(os.path.join(ROOT, "include", "mmloam_hip.h")).read()
    assert re.search(r"#define\s+MML_ABI_VERSION\s+1\b", src)
    assert M.lib().mml_abi_version() == 1


def test_null_context_is_invalid(M):
    L = M.lib()
    T = np.eye(4).reshape(1, 16)
    n = np.zeros(1, np.int32)
    out = np.full(48, 0xA5, np.uint8)
    Tp, np_, outp = (a.ctypes.data_as(C.c_void_p) for a in (T, n, out))
    assert L.mml_cloud_download_registered_batch(None, 0, 1, Tp, outp, 1, np_) == M.MML_ERR_INVALID
    assert L.mml_cloud_download_registered_batch(None, 0, 1, Tp, None, 0, np_) == M.MML_ERR_INVALID
    assert L.mml_cloud_download_registered(None, 0, Tp, outp, 1, np_) == M.MML_ERR_INVALID
    assert (out == 0xA5).all() and n[0] == 0


def test_wrapper_pose_checks(M):
    one = np.arange(16.0).reshape(4, 4)
    # a single pose in either shape, for one slot only
    for T in (one, one.reshape(16), one[None], one.reshape(1, 16), one.tolist()):
        P = M.registered_poses(1, T)
        assert P.shape == (1, 16) and P.dtype == np.float64 and P.flags.c_contiguous
        assert np.array_equal(P[0], np.arange(16.0))
    three = np.arange(48.0).reshape(3, 4, 4)
    for T in (three, three.reshape(3, 16), three.astype(np.float32)):
        P = M.registered_poses(3, T)
        assert P.shape == (3, 16) and np.array_equal(P.reshape(-1), np.arange(48.0))
    bad = [(3, one),                      # one pose for three slots
           (2, three), (4, three),        # count against the pose rows
           (1, three),
           (1, np.zeros((3, 4))),         # not a 4 x 4
           (1, np.zeros(12)),
           (3, np.zeros(48)),             # flat: the rows cannot be told apart from a wrong size
           (2, np.zeros((2, 3, 4))),
           (2, np.zeros((2, 4, 4, 1))),
           (0, np.zeros((0, 4, 4))), (-1, one)]
    for count, T in bad:
        with pytest.raises(ValueError):
            M.registered_poses(count, T)
