"""GPU suite for the world map (mml_world_map_*): slots are filled through mml_cloud_upload with hand-made 48-byte records, so
every point is chosen; every comparison is bit-equal to tests/world_map_ref.py -- the arithmetic is fully defined, there is no
tolerance anywhere."""
import ctypes as C
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rsc

import world_map_ref as R
from conftest import perturbed

pytestmark = pytest.mark.gpu

LEAF = 0.25          # a power of two: the chosen coordinates sit exactly where the C++ check puts them
I4 = np.eye(4)
INFO = ("n_points", "n_kept", "n_nonfinite", "n_out_of_range", "n_masked", "n_new_voxels")


def records(xyz, intensity=None, labels=None):
    """(n, 12) float32 PointXYZINormal records: x y z 1 | time line label 0 | intensity 0 0 0"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rec = np.zeros((len(xyz), 12), np.float32)
    rec[:, :3] = xyz
    rec[:, 3] = 1.0
    rec[:, 6] = 0 if labels is None else np.asarray(labels, np.float32)
    rec[:, 8] = np.arange(len(xyz), dtype=np.float32) * np.float32(0.37) + np.float32(1.5) if intensity is None else np.asarray(intensity, np.float32)
    return rec


def upload(ctx, slot, rec, n_velo=None):
    ctx.cloud_upload(slot, rec, len(rec) // 2 if n_velo is None else n_velo)   # (half in the Velodyne region, half in the Livox one)


def ref_add(ref, map, rec, T, label_mask=7):
    ref.add(map, rec[:, :3], rec[:, 8], T, rec[:, 6].astype(np.int64), label_mask)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_map(ctx, ref, map):
    got, cnt = ctx.world_map_download(map, counts=True)
    exp, ecnt = ref.download(map)
    assert same(cnt, ecnt), (cnt[:8], ecnt[:8])
    assert same(got, exp), np.argwhere(got.view(np.uint32) != exp.view(np.uint32))[:4]
    assert ctx.world_map_size(map) == len(exp)


def info_dict(info):
    return {k: getattr(info, k) for k in INFO}


def voxel_centres(rng, n, span=400):
    """n distinct voxels of LEAF, as points well inside them"""
    ijk = set()
    while len(ijk) < n:
        ijk.add(tuple(int(v) for v in rng.integers(-span, span, 3)))
    return (np.array(sorted(ijk), np.float32) + np.float32(0.5)) * np.float32(LEAF)


@pytest.fixture()
def ctx(M):
    c = M.Context(max_scans=4, max_velo_points=1024, max_livox_points=1024)
    yield c
    c.close()


def poses():
    G = np.eye(4)
    G[:3, :3] = Rsc.from_rotvec([0.3, -0.2, 0.9]).as_matrix()
    G[:3, 3] = [12.5, -7.25, 3.125]
    N = np.array([[1.5, 0.25, -0.125, 4.0], [0.0, -0.75, 2.0, -3.0], [0.3, 0.3, 0.3, 0.1], [0.5, -0.5, 7.0, 2.0]])   # "applied as given"
    return G, N


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_points_in_one_voxel(ctx, n):
    """0 points; 1 point; 63 / 64 / 65 points inside one voxel (the run of one lane around a wave's length)"""
    rng = np.random.default_rng(n)
    rec = records(np.float32(3.0) + rng.random((n, 3), np.float32) * np.float32(0.2))
    upload(ctx, 0, rec)
    ctx.world_map_create(1, LEAF, 16)
    info = ctx.world_map_add(0, [0], I4)
    ref = R.WorldMapRef(LEAF)
    ref_add(ref, 0, rec, I4)
    assert info_dict(info) == ref.info and info.n_voxels_total == (1 if n else 0) and info.n_points == n
    check_map(ctx, ref, 0)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_distinct_voxels_at_workgroup_edges(ctx, n):
    G, _ = poses()
    rec = records(voxel_centres(np.random.default_rng(n), n))
    upload(ctx, 1, rec)
    ctx.world_map_create(1, LEAF, 1024)
    ref = R.WorldMapRef(LEAF)
    for T in (I4, G, I4):    # the second identity call hits every voxel of the first
        info = ctx.world_map_add(1, [0], T)
        ref_add(ref, 0, rec, T)
        assert info.n_kept == n
    assert info.n_new_voxels == 0 and ref.info["n_kept"] == 3 * n
    check_map(ctx, ref, 0)


def test_one_voxel_300_points_over_three_slots(ctx):
    """a run longer than a wave that crosses slot boundaries; the float sums depend on the order (large and small intensities)"""
    rng = np.random.default_rng(7)
    ref = R.WorldMapRef(LEAF)
    for s, n in enumerate((120, 77, 103)):
        inten = np.where(rng.random(n) < 0.3, 1.0e7, 1.0).astype(np.float32) * rng.random(n, np.float32)
        rec = records(np.float32(-5.0) + rng.random((n, 3), np.float32) * np.float32(0.24), inten)
        upload(ctx, s, rec)
        ref_add(ref, 0, rec, I4)
    ctx.world_map_create(1, LEAF, 4)
    info = ctx.world_map_add(0, [0, 0, 0], np.stack([I4] * 3))
    assert info.n_kept == 300 and info.n_new_voxels == 1
    got, cnt = ctx.world_map_download(0, counts=True)
    assert cnt.tolist() == [300]
    check_map(ctx, ref, 0)
    # not vacuous: the same points summed slot 2 first give another float
    back = R.WorldMapRef(LEAF)
    for s in (2, 1, 0):
        d = ctx.scan_download(s)
        back.add_world(0, d["xyzi"])
    assert back.download(0)[1].tolist() == [300] and not same(back.download(0)[0], got)


def edge_coordinates():
    f = np.float32
    hi, lo = f((R.HALF - 1) * LEAF), f(-R.HALF * LEAF)
    below0 = np.nextafter(f(0), f(-1))
    vals = [f(-0.0), f(0.0), f(-LEAF), below0, np.nextafter(f(-LEAF), f(-1e9)), np.nextafter(f(LEAF), f(0)), f(LEAF), hi, -hi, lo,
            np.nextafter(f(R.HALF * LEAF), f(0))]
    out_of_range = [f(R.HALF * LEAF), np.nextafter(lo, f(-1e9)), f(1.0e30), f(-1.0e30), f(3.0e38)]
    return vals, out_of_range


def test_voxel_edges_identity_pose(ctx):
    """the coordinates of the C++ check on each axis and sign, just inside and just outside the range; NaN / inf coordinates and
    intensity; every count of `info`"""
    vals, oor = edge_coordinates()
    pts, inten = [], []
    for axis in range(3):
        for v in vals + oor:
            p = [1.0, 1.0, 1.0]
            p[axis] = v
            pts.append(p)
            inten.append(2.0)
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = [1.0, 1.0, 1.0]
            p[axis] = bad
            pts.append(p)
            inten.append(2.0)
        pts.append([1.0, 1.0, 1.0])
        inten.append(bad)
    pts.append([np.nan, 1.0e30, 1.0])    # not finite is counted before out of range
    inten.append(1.0)
    rec = records(pts, inten)
    upload(ctx, 0, rec)
    ctx.world_map_create(1, LEAF, 256)
    info = ctx.world_map_add(0, [0], I4)
    ref = R.WorldMapRef(LEAF)
    ref_add(ref, 0, rec, I4)
    assert ref.info["n_out_of_range"] == 3 * len(oor) and ref.info["n_nonfinite"] == 13 and ref.info["n_kept"] == 3 * len(vals)
    assert info_dict(info) == ref.info
    check_map(ctx, ref, 0)


def test_voxel_edges_through_poses(ctx):
    """the same coordinates through a rotation with translation and through a non-orthonormal upper block (applied as given)"""
    vals, oor = edge_coordinates()
    pts = [[a, b, c] for a in vals[:7] for b in (vals[0], vals[3], vals[6]) for c in (vals[2], vals[5])]
    pts += [[v, 0.5, -0.5] for v in vals + oor] + [[0.5, v, 0.5] for v in vals + oor] + [[np.nan, 0, 0], [0, np.inf, 0]]
    rec = records(pts)
    upload(ctx, 2, rec)
    ctx.world_map_create(2, LEAF, 1024)
    G, N = poses()
    ref = R.WorldMapRef(LEAF)
    for m, T in ((0, G), (1, N)):
        info = ctx.world_map_add(2, [m], T)
        before = dict(ref.info)
        ref_add(ref, m, rec, T)
        assert info_dict(info) == {k: ref.info[k] - before[k] for k in INFO}
        assert info.n_kept > 40 and info.n_out_of_range > 0 and info.n_nonfinite >= 2      # (3e38 through a pose may overflow to inf)
    check_map(ctx, ref, 0)
    check_map(ctx, ref, 1)


def test_the_empty_markers_voxel_is_out_of_range(M):
    """map 1023 of 1024 at a tiny capacity; its voxel (2^17-1)^3 would carry the key that marks a free position"""
    c = M.Context(max_scans=1, max_velo_points=64, max_livox_points=64)
    try:
        hi = np.float32((R.HALF - 1) * LEAF)
        rec = records([[hi, hi, hi], [hi, hi, hi - np.float32(LEAF)], [1, 2, 3], [1.01, 2.01, 3.01], [-hi, -hi, -hi]])
        upload(c, 0, rec)
        c.world_map_create(1024, LEAF, 4)
        ref = R.WorldMapRef(LEAF)
        info = c.world_map_add(0, [1023], I4)
        ref_add(ref, 1023, rec, I4)
        assert info_dict(info) == ref.info and info.n_out_of_range == 1 and info.n_kept == 4 and info.n_new_voxels == 3
        info = c.world_map_add(0, [1023], I4)
        ref_add(ref, 1023, rec, I4)
        assert info.n_new_voxels == 0 and info.n_voxels_total == 3
        check_map(c, ref, 1023)
        assert c.world_map_size(1022) == 0 and c.world_map_size(0) == 0 and c.world_map_size(-1) == 3
        c.world_map_reset(1023)
        assert c.world_map_size(-1) == 0 and len(c.world_map_download(1023)) == 0
        info = c.world_map_add(0, [1022], I4)      # in map 1022 the same voxel is an ordinary one
        assert info.n_kept == 5 and info.n_new_voxels == 4 and info.n_out_of_range == 0
    finally:
        c.close()


@pytest.mark.parametrize("capacity", [1, 4, 64])
def test_table_filled_to_capacity_then_every_voxel_hit_again(ctx, capacity):
    """random distinct voxels into 2 x capacity positions: collisions and the wrap at the table's end are certain (asserted through
    the host hash); then a second point into every voxel; then one voxel more: MML_ERR_CAPACITY and nothing changed"""
    M = importlib.import_module("multi-modal-loam_amd")
    rng = np.random.default_rng(100 + capacity)
    slots = R.table_slots(capacity)
    cen = voxel_centres(rng, capacity + 1)
    if capacity > 1:
        first = [R.hash_position(R.pack(0, *[int(np.floor(v / LEAF)) for v in p]), slots) for p in cen[:capacity]]
        assert len(set(first)) < capacity                                    # at least two keys start at one position
    rec = records(cen[:capacity])
    upload(ctx, 0, rec)
    ctx.world_map_create(1, LEAF, capacity)
    ref = R.WorldMapRef(LEAF)
    info = ctx.world_map_add(0, [0], I4)
    ref_add(ref, 0, rec, I4)
    assert info.n_new_voxels == capacity and info.n_voxels_total == capacity
    check_map(ctx, ref, 0)
    rec2 = records(cen[:capacity][::-1] + np.float32(0.01), intensity=np.full(capacity, 9.0))
    upload(ctx, 1, rec2)
    info = ctx.world_map_add(1, [0], I4)
    ref_add(ref, 0, rec2, I4)
    assert info.n_new_voxels == 0 and info.n_kept == capacity
    check_map(ctx, ref, 0)
    # capacity + 1: refused, the table byte for byte what it was, and a legal call still works
    before = ctx.world_map_download(0, counts=True)
    upload(ctx, 2, records(np.concatenate([cen[:1], cen[capacity:]])))      # one voxel that is held and one new one
    with pytest.raises(M.MmlError) as e:
        ctx.world_map_add(2, [0], I4)
    assert e.value.code == M.MML_ERR_CAPACITY and str(capacity) in str(e.value)
    after = ctx.world_map_download(0, counts=True)
    assert same(before[0], after[0]) and same(before[1], after[1]) and ctx.world_map_size(0) == capacity == ctx.world_map_size(-1)
    info = ctx.world_map_add(1, [0], I4)
    ref_add(ref, 0, rec2, I4)
    assert info.n_new_voxels == 0
    check_map(ctx, ref, 0)


def test_keys_that_start_at_the_last_table_position(ctx):
    """keys chosen through the host hash to start at the table's last position: all but one wrap to its front"""
    capacity = 8
    slots = R.table_slots(capacity)
    chosen, i = [], 0
    while len(chosen) < 5:
        if R.hash_position(R.pack(0, i, -i, 3), slots) == slots - 1:
            chosen.append([i, -i, 3])
        i += 1
    rec = records((np.array(chosen, np.float32) + np.float32(0.5)) * np.float32(LEAF))
    upload(ctx, 0, rec)
    ctx.world_map_create(1, LEAF, capacity)
    ref = R.WorldMapRef(LEAF)
    for _ in range(2):
        info = ctx.world_map_add(0, [0], I4)
        ref_add(ref, 0, rec, I4)
    assert sorted(ref.vox) == sorted(R.pack(0, *c) for c in chosen) and info.n_new_voxels == 0 and info.n_voxels_total == 5
    check_map(ctx, ref, 0)


def test_maps_do_not_mix_skip_and_reset(ctx):
    rng = np.random.default_rng(5)
    G, _ = poses()
    recs = [records(voxel_centres(rng, 40, span=3) + rng.random((40, 3), np.float32) * np.float32(0.1)) for _ in range(3)]
    for s in range(3):
        upload(ctx, s, recs[s])
    ctx.world_map_create(3, LEAF, 512)
    ref = R.WorldMapRef(LEAF)
    info = ctx.world_map_add(0, [0, -1, 1], np.stack([I4, G, I4]))           # slot 1 is skipped
    ref_add(ref, 0, recs[0], I4)
    ref_add(ref, 1, recs[2], I4)
    assert info_dict(info) == ref.info and info.n_points == 80
    info = ctx.world_map_add(0, [1, 0, -1], np.stack([I4, G, I4]))           # the same voxels into the other map: they do not mix
    ref_add(ref, 1, recs[0], I4)
    ref_add(ref, 0, recs[1], G)
    for m in (0, 1, 2):
        check_map(ctx, ref, m)
    assert ctx.world_map_size(2) == 0 and ctx.world_map_size(-1) == ref.size()
    assert ctx.world_map_add(0, [-1, -1], np.stack([I4, I4])).n_voxels_total == ref.size()     # nothing takes part
    keep = ctx.world_map_download(1, counts=True)
    ctx.world_map_reset(0)
    ref.reset(0)
    again = ctx.world_map_download(1, counts=True)
    assert same(keep[0], again[0]) and same(keep[1], again[1])
    check_map(ctx, ref, 0)
    check_map(ctx, ref, 1)
    assert ctx.world_map_size(0) == 0 and ctx.world_map_size(-1) == ref.size(1)
    info = ctx.world_map_add(2, [0], G)                                       # the table works on after the rebuild
    ref_add(ref, 0, recs[2], G)
    info = ctx.world_map_add(0, [1], I4)
    ref_add(ref, 1, recs[0], I4)
    check_map(ctx, ref, 0)
    check_map(ctx, ref, 1)
    ctx.world_map_reset(-1)
    assert [ctx.world_map_size(m) for m in (-1, 0, 1, 2)] == [0, 0, 0, 0] and len(ctx.world_map_download(1)) == 0
    info = ctx.world_map_add(1, [2], I4)
    fresh = R.WorldMapRef(LEAF)
    ref_add(fresh, 2, recs[1], I4)
    assert info_dict(info) == fresh.info
    check_map(ctx, fresh, 2)


def test_batching_guarantee(M):
    """three slots in one call, in three calls, split 2 + 1: downloads, counts and summed info equal; five fresh contexts each
    (which position a key lands in may differ from run to run, what a call returns may not)"""
    rng = np.random.default_rng(11)
    G, N = poses()
    T = np.stack([I4, G, N])
    base = voxel_centres(rng, 50, span=2)
    recs = []
    for s in range(3):     # the three slots share voxels (under the identity) and carry order-sensitive intensities
        pick = base[rng.integers(0, len(base), 333 + s)] + (rng.random((333 + s, 3), np.float32) - np.float32(0.5)) * np.float32(0.2)
        inten = np.where(rng.random(len(pick)) < 0.2, 3.0e7, 1.0).astype(np.float32) * rng.random(len(pick), np.float32)
        recs.append(records(pick, inten, labels=rng.integers(0, 3, len(pick))))
    ref = R.WorldMapRef(LEAF)
    for s in range(3):
        ref_add(ref, s % 2, recs[s], T[s])
    maps = [0, 1, 0]
    seen = set()
    for rep in range(5):
        for split in ((3,), (1, 1, 1), (2, 1)):
            c = M.Context(max_scans=3, max_velo_points=256, max_livox_points=256)
            try:
                for s in range(3):
                    upload(c, s, recs[s])
                c.world_map_create(2, LEAF, 4096)
                total, s0 = dict.fromkeys(INFO, 0), 0
                for k in split:
                    info = c.world_map_add(s0, maps[s0:s0 + k], T[s0:s0 + k])
                    for key in INFO:
                        total[key] += getattr(info, key)
                    s0 += k
                assert total == ref.info and info.n_voxels_total == ref.size()
                check_map(c, ref, 0)
                check_map(c, ref, 1)
                seen.add(c.world_map_download(0).tobytes() + c.world_map_download(1).tobytes())
            finally:
                c.close()
    assert len(seen) == 1


def test_label_mask_and_refusals(ctx):
    M = importlib.import_module("multi-modal-loam_amd")
    rng = np.random.default_rng(3)
    labels = np.arange(90) % 3
    rec = records(voxel_centres(rng, 30, span=2)[np.arange(90) % 30] + rng.random((90, 3), np.float32) * np.float32(0.1), labels=labels)
    upload(ctx, 0, rec)
    with pytest.raises(M.MmlError) as e:
        ctx.world_map_add(0, [0], I4)                                          # no map yet
    assert e.value.code == M.MML_ERR_STATE
    for bad in (dict(n_maps=0), dict(n_maps=1025), dict(leaf=0.0), dict(leaf=-1.0), dict(leaf=np.inf), dict(leaf=np.nan), dict(capacity_voxels=0)):
        args = dict(n_maps=4, leaf=LEAF, capacity_voxels=256)
        args.update(bad)
        with pytest.raises(M.MmlError) as e:
            ctx.world_map_create(**args)
        assert e.value.code == M.MML_ERR_INVALID, bad
    ctx.world_map_create(4, LEAF, 256)
    with pytest.raises(M.MmlError) as e:
        ctx.world_map_create(4, LEAF, 256)
    assert e.value.code == M.MML_ERR_STATE
    ref = R.WorldMapRef(LEAF)
    for m, mask in enumerate((1, 2, 4, 6)):
        info = ctx.world_map_add(0, [m], I4, label_mask=mask)
        before = dict(ref.info)
        ref_add(ref, m, rec, I4, mask)
        assert info_dict(info) == {k: ref.info[k] - before[k] for k in INFO}
        assert info.n_masked == 30 * (3 - bin(mask).count("1")) and info.n_kept == 90 - info.n_masked
    for m in range(4):
        check_map(ctx, ref, m)
    ctx.world_map_reset(0)
    ref.reset(0)
    ctx.world_map_add(0, [0], I4, label_mask=7)
    ref_add(ref, 0, rec, I4, 7)
    check_map(ctx, ref, 0)

    def state():
        return [tuple(a.tobytes() for a in ctx.world_map_download(m, counts=True)) for m in range(4)] + [ctx.world_map_size(-1)]

    before = state()
    L, h = M.lib(), ctx._h
    one, T1 = np.zeros(1, np.int32), np.ascontiguousarray(I4.reshape(1, 16))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    big = np.zeros(70000, np.int32)
    refusals = [
        L.mml_world_map_add(h, 0, 1, p(one), p(T1), 0, None),                 # mask 0
        L.mml_world_map_add(h, 0, 1, p(one), p(T1), 8, None),                 # no bit of the three
        L.mml_world_map_add(h, -1, 1, p(one), p(T1), 7, None),                # slot ranges
        L.mml_world_map_add(h, 4, 1, p(one), p(T1), 7, None),
        L.mml_world_map_add(h, 3, 2, p(big), p(np.zeros((2, 16))), 7, None),
        L.mml_world_map_add(h, 0, 0, p(one), p(T1), 7, None),                 # count
        L.mml_world_map_add(h, 0, 65536, p(big), p(np.zeros((65536, 16))), 7, None),
        L.mml_world_map_add(h, 0, 1, p(np.array([4], np.int32)), p(T1), 7, None),    # map numbers
        L.mml_world_map_add(h, 0, 1, p(np.array([-2], np.int32)), p(T1), 7, None),
        L.mml_world_map_add(h, 0, 1, p(one), None, 7, None),                  # NULL T_wl
        L.mml_world_map_add(h, 0, 1, None, p(T1), 7, None),
        L.mml_world_map_reset(h, 4), L.mml_world_map_reset(h, -2),
    ]
    assert refusals == [M.MML_ERR_INVALID] * len(refusals)
    assert state() == before
    ctx.world_map_destroy()
    with pytest.raises(M.MmlError) as e:
        ctx.world_map_size(0)
    assert e.value.code == M.MML_ERR_STATE
    ctx.world_map_create(1, 0.5, 8)                                            # a new one after the destroy
    assert ctx.world_map_size(-1) == 0


def _sequence_inputs(synth, w, rounds):
    out = []
    for i in range(rounds):
        k = (20, 60)[w] + (4, 5)[w] * i
        v, l = synth.velo_scan(k, n_az=450, motion=True), synth.livox_scan(k, n=6000, motion=True)
        dR, dt = synth.sweep_motion(k)
        Tp = perturbed(synth.pose_matrix(k), dt=(0.02, -0.015, 0.01), rotvec=(0.002, -0.001, 0.003))
        out.append((v, l, dR, dt, Tp[:3, 3].copy(), Rsc.from_matrix(Tp[:3, :3]).as_quat()))
    return out


def test_batch_odometry_loop(M, synth):
    """BatchLidarOdometry(world_map=...) over a few scans of the synthetic scene: every sequence's map equals the restatement fed
    with cloud_download_registered of the same slots and poses; the poses equal those of a run without the map, bitwise; the
    caller's fast-rotation flag keeps a scan out"""
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    W, rounds = 2, 3
    inputs = [_sequence_inputs(synth, w, rounds) for w in range(W)]
    runs = {}
    for wm in (None, (0.2, 1 << 16)):
        c = M.Context(max_scans=W, max_map_points=1 << 19)
        try:
            bat = odometry.BatchLidarOdometry(c, W, lidar_mode=2, world_map=wm)
            ref, poses_out, published = R.WorldMapRef(0.2), [], 0
            for i in range(rounds):
                for w in range(W):
                    c.scan_upload(w, inputs[w][i][0], inputs[w][i][1])
                c.extract(0, W)
                c.undistort(0, W, np.stack([inputs[w][i][2].reshape(9) for w in range(W)]), np.stack([inputs[w][i][3] for w in range(W)]))
                fast = [i == 2, False]
                P, Q, grew = bat.estimate_lidar_pose(list(range(W)), np.stack([inputs[w][i][4] for w in range(W)]),
                                                     np.stack([inputs[w][i][5] for w in range(W)]), fast_rotation=fast)
                poses_out.append((P.tobytes(), Q.tobytes(), tuple(grew)))
                if wm:
                    for w in range(W):
                        if not bat.seq[w].fail_detected and not fast[w]:
                            ref.add_records(w, c.cloud_download_registered(w, 1, bat.seq[w].last_T)[0])
                            published += 1
            if wm:
                assert 3 <= published <= 2 * rounds - 1          # (sequence 0 in round 2: fast rotation)
                for w in range(W):
                    got = bat.world_map(w)
                    exp, _ = ref.download(w)
                    assert len(exp) > 1000 and same(got, exp)
                with pytest.raises(ValueError):
                    bat.world_map(W)
            else:
                with pytest.raises(ValueError):
                    bat.world_map(0)
            runs[wm is not None] = poses_out
        finally:
            c.close()
    assert runs[True] == runs[False]
