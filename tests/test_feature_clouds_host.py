"""CPU suite for the feature node's message (mml_feature_clouds_download / _batch): the C-ABI surface, and the oracle property the
device test (tests/test_feature_clouds_gpu.py) relies on -- what separates the reference's four per-sensor feature clouds from a
label filter of the fused cloud, which is why the call exists."""
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from feature_clouds_expect import cached

NAMES = ("mml_feature_clouds_download", "mml_feature_clouds_download_batch")


def test_declared_in_the_header_and_exported(M):
    src = open(os.path.join(ROOT, "include", "mmloam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = re.findall(r"\bint\s+(mml_[a-z0-9_]+)\s*\(", src)
    nm = subprocess.run(["nm", "-D", "--defined-only", M.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NAMES:
        assert declared.count(name) == 1, name
        assert name in exported, name
    assert M.lib().mml_feature_clouds_download_batch(None, 0, 1, None, 0, None) == M.MML_ERR_INVALID
    assert M.POINTXYZINORMAL_DTYPE.itemsize == 48 and len(M.FEATURE_CLOUD_NAMES) == 6 and callable(M.Context.feature_clouds)
    # the bucketing block the device test sizes its scans by is the library's
    internal = open(os.path.join(os.path.dirname(M.LIB_PATH), "csrc", "mml_internal.h")).read()
    assert re.search(r"#define\s+MML_OP_BLK\s+%d\b" % M.ASSIGN_BLOCK_POINTS, internal)


def test_label_filter_of_the_fused_cloud_is_not_the_feature_clouds(O):
    """far_th = 8 m on a full scan.  Against the reference's clouds, a label filter of the fused cloud [velo_combine ;
    livox_combine] -- all a caller of the parent library could do --
      * loses the labelled Livox points beyond far_th (the Livox corner / surf clouds are cropped near only, :925 / :933) and
        nothing else: what is left of the reference cloud when those are taken out is the filter's result, record for record;
      * carries intensity 0 in the Velodyne part (:1254-1256) where the reference's clouds, copied first (:1244-1252), carry
        the sensor's -- and is otherwise the same records.
    The order is the third thing the issue names; in the ORACLE's fused cloud there is none to lose: it is handed out in raw
    order (kept points in input order), so the filter is a subsequence of the raw cloud like the reference's clouds.  The
    line-bucketed order is the device's STORAGE order, which is why the device walks the raw line ids to restore it; that is
    checked on the device."""
    far = 8.0
    v, l, e = cached(14, 1800, 24000, False, far)
    assert e["far_labelled"] >= 10
    # Livox: filter of the fused part = the reference cloud without its far points, same order
    lf = e["livox_fused"]
    n_lost = 0
    for c, name in ((1, "livox_corner"), (2, "livox_surface")):
        filt = lf[lf[:, 6] == c]
        ref = e[name]
        d2 = (ref[:, 0] * ref[:, 0] + ref[:, 1] * ref[:, 1]) + ref[:, 2] * ref[:, 2]
        near_part = ref[~(d2 > np.float32(far) * np.float32(far))]
        assert np.array_equal(filt.view(np.uint32), near_part.view(np.uint32)), name
        n_lost += len(ref) - len(filt)
    assert n_lost == e["far_labelled"]
    assert e["counts"][2] == len(e["livox_corner"]) and e["counts"][3] == len(e["livox_surface"])
    # Velodyne: same records but for the intensity
    vf = e["velo_fused"]
    for c, name in ((1, "velo_corner"), (2, "velo_surface")):
        filt = vf[vf[:, 6] == c]
        ref = e[name]
        assert len(filt) == len(ref) == e["counts"][c - 1]
        assert (filt[:, 8] == 0).all() and (ref[:, 8] != 0).any(), name
        same = [k for k in range(12) if k != 8]
        assert np.array_equal(filt[:, same].view(np.uint32), ref[:, same].view(np.uint32)), name
    # raw order: the reference's Velodyne clouds are subsequences of the input, intensity included
    keys = [r.tobytes() for r in np.ascontiguousarray(v)]
    for name in ("velo_corner", "velo_surface"):
        it = iter(keys)
        want = [r.tobytes() for r in np.ascontiguousarray(e[name][:, [0, 1, 2, 8]])]
        assert all(any(k == w for k in it) for w in want), name
