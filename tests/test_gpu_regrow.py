"""The grow-only device buffers of a context (csrc/mml_mem.h) replaced while the context is live: a context that saw a small
call before the large one must give, byte for byte, what a fresh context gives that only ever saw the large one.

Not repeated here, because existing tests already use these lazily allocated groups many times in one context:
the cube store (tests/test_gpu_parity.py::test_global_cube_store_matches_oracle, ten increments) and the frame-parallel
window-solve state (tests/test_gpu_multi.py::test_frame_parallel_window_solve_equals_the_sequential_kernel, twelve solves)."""
import numpy as np
import pytest

from conftest import perturbed, shifted

pytestmark = pytest.mark.gpu


def _pair(M):
    return M.Context(max_scans=2, max_map_points=8192), M.Context(max_scans=2, max_map_points=8192)


def _same_scan(a, b):
    assert a["info"].n_points == b["info"].n_points and a["info"].n_velo == b["info"].n_velo
    for key in ("xyzi", "reltime", "ring", "label"):
        assert a[key].tobytes() == b[key].tobytes(), key


def test_wire_stage_regrows(M, scene):
    fr = scene["frames"][0]
    v, l = fr["velo"], fr["livox"]
    step = 22  # the velodyne driver's PointCloud2 record: x y z intensity float32, ring uint16, time float32
    raw = np.zeros((len(v), step), np.uint8)
    raw[:, 0:16] = v.view(np.uint8).reshape(len(v), 16)
    lw = np.ascontiguousarray(np.ascontiguousarray(l).view(np.uint8).reshape(len(l), 20)[:, :19])
    grown, fresh = _pair(M)
    try:
        grown.scan_upload_wire(0, raw[:64].reshape(-1), 64, step, 0, 4, 8, 12, lw[:64].reshape(-1), 64)   # stage: 64 x (22 + 19) bytes
        grown.extract(0, 1)
        for c in (grown, fresh):
            c.scan_upload_wire(0, raw.reshape(-1), len(v), step, 0, 4, 8, 12, lw.reshape(-1), len(l))
            c.extract(0, 1)
        want = fresh.scan_download(0)
        assert want["info"].n_points > 20000
        _same_scan(grown.scan_download(0), want)
        # the labelled cloud back in through mml_cloud_upload: 64 records, then all of them
        rec = fresh.scan_download_pointxyzinormal(0)
        nv = want["info"].n_velo
        small, fresh2 = _pair(M)
        try:
            small.cloud_upload(1, rec[:64], 64)
            for c in (small, fresh2):
                c.cloud_upload(1, rec, nv)
            _same_scan(small.scan_download(1), fresh2.scan_download(1))
        finally:
            small.close()
            fresh2.close()
    finally:
        grown.close()
        fresh.close()


def test_global_grid_group_regrows(M, cube_scene):
    cs = cube_scene
    assert len(cs["surf_global"]) > 1024  # beyond the 1024-point floor of the group: the second call replaces it
    fr = cs["frames"][0]
    T = shifted(perturbed(fr["T_gt"]), cs["shift"])[None]
    grown, fresh = _pair(M)
    try:
        for name, kind in (("corner", 0), ("surf", 1)):
            grown.map_set_global(kind, cs[name + "_global"][:100], cs[name + "_cube"][:100])
        out = []
        for c in (grown, fresh):
            for name, kind in (("corner", 0), ("surf", 1)):
                c.map_set_local(kind, cs[name + "_local"])
                c.map_set_global(kind, cs[name + "_global"], cs[name + "_cube"])
                c.features_upload(0, kind, fr[name])
            c.associate(0, 1, T, 25.0)
            out.append([c.factors_download(0, kind) for kind in range(2)])
        for kind in range(2):
            (ra, sa), (rb, sb) = out[0][kind], out[1][kind]
            assert len(sb) > 50 and np.array_equal(sa, sb) and ra.tobytes() == rb.tobytes()
    finally:
        grown.close()
        fresh.close()


def test_sort_scratch_regrows(M, scene):
    maps = (scene["corner_map"], scene["surf_map"])
    fr = scene["frames"][1]
    q = (scene["surf_map"][:8] + np.float32(0.05)).astype(np.float32)
    grown, fresh = _pair(M)
    try:
        grown.map_set_local(0, maps[0][:100])
        grown.map_set_local(1, maps[1][:300])      # sort scratch for 300 points
        out = []
        for c in (grown, fresh):
            c.map_set_local(0, maps[0])
            c.map_set_local(1, maps[1])            # ... for 5 k
            res = [c.knn5(kind, q) for kind in range(2)]
            c.features_upload(0, 0, fr["corner"])
            c.features_upload(0, 1, fr["surf"])
            for step in range(2):                  # the voxel filter's sort and scan share the scratch
                res.append(c.map_increment_local(0, perturbed(fr["T_gt"], dt=(0.3 * step, 0.0, 0.0))))
            res.append([c.map_local_download(kind) for kind in range(2)])
            out.append(res)
        a, b = out
        for kind in range(2):
            assert np.array_equal(a[kind][0], b[kind][0]) and a[kind][1].tobytes() == b[kind][1].tobytes()
            assert (b[kind][0] >= 0).all()
            assert len(b[4][kind]) > 100 and a[4][kind].tobytes() == b[4][kind].tobytes()
        assert tuple(a[2]) == tuple(b[2]) and tuple(a[3]) == tuple(b[3])
    finally:
        grown.close()
        fresh.close()
