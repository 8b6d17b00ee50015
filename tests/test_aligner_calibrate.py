"""The aligner's start-up calibration, without a GPU: the C-ABI declares the three calls and two structs (ABI version unchanged),
the Python wrappers exist, and the GPU tests' own numpy reference (tests/calibrate_checks.py) agrees with the oracle."""
import ctypes as C
import os
import re

import numpy as np

import calibrate_checks as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "mmloam_hip.h")).read()


def test_header_declares_the_calls_and_structs():
    h = re.sub(r"\s+", " ", header())
    assert "#define MML_ABI_VERSION 1 " in h + " "
    assert re.search(r"typedef struct \{ int max_iterations;.*?double transformation_epsilon;.*?double max_correspondence_distance;.*?\} "
                     r"mml_gicp_opts;", h)
    assert re.search(r"typedef struct \{ int n_hori_in, n_velo_in;.*?int n_hori_ds, n_velo_ds;.*?int hori_unfiltered, velo_unfiltered;.*?"
                     r"mml_gicp_info gicp; \} mml_calib_info;", h)
    assert re.search(r"int mml_gicp_align_opts\(mml_ctx\* ctx, const float\* src_xyz, int n_src, const float\* tgt_xyz, int n_tgt, "
                     r"const mml_gicp_opts\* opts, float\* T_inout, int\* converged, mml_gicp_info\* info", h)
    assert re.search(r"int mml_cloud_crop_voxel\(mml_ctx\* ctx, const float\* xyzi, int n, float far_th, float leaf, float\* out_xyzi, "
                     r"int capacity, int\* n_out, int\* unfiltered", h)
    assert re.search(r"int mml_aligner_calibrate\(mml_ctx\* ctx, const float\* hori_xyzi, int n_hori, const float\* velo_xyzi, int n_velo, "
                     r"float\* hori_tf /\* 16 \*/, float\* velo_hori_tf /\* 16 \*/, int\* converged, mml_calib_info\* info", h)
    # the existing declarations are where they were
    assert "int mml_gicp_align(mml_ctx* ctx, const float* src_xyz, int n_src, const float* tgt_xyz, int n_tgt, float* T_inout, int* converged," in h


def test_wrappers_and_structs_exist(M):
    for name in ("gicp_align_opts", "cloud_crop_voxel", "aligner_calibrate"):
        assert callable(getattr(M.Context, name)), name
    assert [f[0] for f in M.GicpOpts._fields_] == ["max_iterations", "transformation_epsilon", "max_correspondence_distance"]
    assert C.sizeof(M.GicpOpts) == 24                                        # int, pad, double, double
    assert C.sizeof(M.CalibInfo) == 24 + C.sizeof(M.GicpInfo) == 48
    assert M.CalibInfo.gicp.offset == 24


def test_library_exports_the_symbols(M):
    L = M.lib()                                                              # (loading needs no device)
    for name in ("mml_gicp_align_opts", "mml_cloud_crop_voxel", "mml_aligner_calibrate"):
        assert hasattr(L, name), name


def test_crop_helper_meets_the_oracles_input_contract(O):
    """crop_far hands oracle.voxel_downsample what it takes -- C-ordered float32 rows that survive the oracle's own float32
    conversion unchanged -- keeps order, and cuts strictly above far_th^2 in float arithmetic."""
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-40.0, 40.0, (500, 3))
    cloud = K.with_intensity(xyz, 3)
    c = K.crop_far(cloud, 50.0)
    assert c.dtype == np.float32 and c.flags.c_contiguous and 0 < len(c) < len(cloud)
    assert np.ascontiguousarray(c[:, :3], dtype=np.float32).tobytes() == c[:, :3].copy().tobytes()
    r2 = (cloud[:, 0].astype(np.float64) ** 2 + cloud[:, 1].astype(np.float64) ** 2) + cloud[:, 2].astype(np.float64) ** 2
    sure = np.abs(r2 - 2500.0) > 1e-2                                        # away from the float rounding of the boundary
    kept = np.zeros(len(cloud), bool)
    kept[[int(np.flatnonzero((cloud == row).all(1))[0]) for row in c]] = True
    assert np.array_equal(kept[sure], (r2 <= 2500.0)[sure])
    idx = [int(np.flatnonzero((cloud == row).all(1))[0]) for row in c]
    assert idx == sorted(idx)
    # a leaf far below the point spacing: every point its own voxel, so the oracle returns the cropped points themselves (x / 1 = x)
    lattice = np.stack(np.meshgrid(np.arange(4), np.arange(3), np.arange(2), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    lat = K.crop_far(K.with_intensity(lattice, 4), 3.5)
    out = O.voxel_downsample(lat[:, :3], 0.25)
    assert len(out) == len(lat) and {r.tobytes() for r in out} == {np.ascontiguousarray(r).tobytes() for r in lat[:, :3]}
    on = np.array([[30.0, 40.0, 0.0, 1.0], [30.0, np.nextafter(np.float32(40.0), np.float32(50.0)), 0.0, 2.0]], np.float32)
    assert len(K.crop_far(on, 50.0)) == 1


def test_voxel_mean4_is_the_oracles_filter_with_intensity(O):
    """voxel_mean4's x, y, z are oracle.voxel_downsample's bits (host_crop_voxel asserts it) at the GPU tests' shapes, so its
    fourth column is the mean over the oracle's groups in the oracle's order; the overflow refusal is the oracle's too."""
    for seed, n, leaf in ((1, 1, 0.5), (2, 257, 0.5), (3, 1500, 0.2), (4, 300, 0.05)):
        rng = np.random.default_rng(seed)
        cloud = K.with_intensity(K.corner_cloud(rng, n) - np.array([1.5, 2.0, 0.5]), seed)
        ref, unf = K.host_crop_voxel(O, cloud, 3.0, leaf)
        assert not unf and len(ref) <= n
    wide = K.with_intensity(np.array([[49.9, 0, 0], [-49.9, 0, 0], [0, 49.9, 0], [0, -49.9, 0], [0, 0, 49.9], [0, 0, -49.9], [1, 1, 1]]), 5)
    ref, unf = K.host_crop_voxel(O, wide, 50.0, 0.05)
    assert unf and ref.tobytes() == wide.tobytes()
    ref, unf = K.host_crop_voxel(O, wide, 50.0, 0.5)
    assert not unf and len(ref) == 7
