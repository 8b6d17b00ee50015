"""The shared pieces of csrc/voxel_sort_dev.h -- the bounding-box tail, the heads kernel, the run loop, the sort and scan helpers --
through the public calls that reach them, at the smallest shapes at which a 256-thread kernel can go wrong, bit for bit against the
oracle's filter / search:
  mml_cloud_crop_voxel                 k_cv_bbox, 64-bit keys, limit CV_DROPPED, the four-field run sum, a side call's own scratch
  features_upload + map_increment_local  the increment chain with one map (k_inc_concat_bbox, kind << 32 | voxel keys, the three-field run
                                         sum, the context's sort_tmp); the rebuilt grids (map_assoc.hip's mml_build_grids, two segments) are
                                         then read through knn5
  map_set_local + knn5                  map_assoc.hip's grid build alone (k_bbox, one cloud, 32-bit keys)
  mml_time_offset_search                k_tofs_box, the box decoded on the host, the sort scratch carved out of the call's block
The clouds come from calibrate_checks' generators.  Every case takes well under a second."""
import numpy as np
import pytest

import calibrate_checks as K

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 513]   # one lane, one workgroup exactly, one over, two workgroups plus one
FAR = 50.0


@pytest.fixture(scope="module")
def ctx(M):
    c = M.Context(max_scans=1)
    yield c
    c.close()


# ---- the clouds: name -> f(leaf) -> n x 3 float32 ----------------------------------------------------------------------------
def room(seed, n):
    return (K.corner_cloud(np.random.default_rng(seed), n) - np.array([1.5, 2.0, 0.5])).astype(np.float32)   # negative coordinates too


def run_across_the_workgroup_edge(leaf):
    """A 20-voxel-wide sheet whose voxel indices are 0 .. 350: voxels 0 .. 249 hold one point each, voxel 250 holds 12 (sorted
    positions 250 .. 261: the run's head reads its left neighbour inside workgroup 0, the run loop walks across position
    255 -> 256), voxels 251 .. 350 one each; input shuffled."""
    rng = np.random.default_rng(5)
    cell = np.concatenate([np.arange(250), np.full(12, 250), np.arange(251, 351)])
    p = np.stack([(cell % 20 - 10 + rng.uniform(0.2, 0.8, len(cell))) * leaf, (cell // 20 - 9 + rng.uniform(0.2, 0.8, len(cell))) * leaf,
                  -rng.uniform(0.2, 0.8, len(cell)) * leaf], 1)
    return p[rng.permutation(len(p))].astype(np.float32)


def one_voxel(leaf):
    return (np.random.default_rng(6).uniform(0.1, 0.9, (300, 3)) * leaf - np.array([3 * leaf, 0, leaf])).astype(np.float32)


def every_point_its_own_voxel(leaf):
    g = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing="ij"), -1).reshape(-1, 3)   # 343 cells
    rng = np.random.default_rng(7)
    return ((g + rng.uniform(0.2, 0.8, g.shape)) * leaf)[rng.permutation(len(g))].astype(np.float32)


def extremum_last(sign):
    """513 points: the x extremum is attained only by the last point, the only one of the last workgroup (its other lanes hold
    +-inf when the box is reduced)."""
    def make(leaf):
        p = room(8, 513)
        p[-1, 0] = np.float32(sign * 9.75)
        assert (sign * p[:-1, 0]).max() < 9.0
        return p
    return make


SHAPES = {"run_across_edge": run_across_the_workgroup_edge, "one_voxel": one_voxel, "own_voxels": every_point_its_own_voxel,
          "max_x_last": extremum_last(+1), "min_x_last": extremum_last(-1)}
SHAPES.update({"n%d" % n: (lambda leaf, n=n: room(20 + n, n)) for n in SIZES})


# ---- mml_cloud_crop_voxel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_crop_voxel_matches_the_oracle(ctx, O, name):
    leaf = 0.5
    cloud = K.with_intensity(SHAPES[name](leaf), 3)
    ref, ref_unf = K.host_crop_voxel(O, cloud, FAR, leaf)
    out, unf = ctx.cloud_crop_voxel(cloud, FAR, leaf)
    print(name, len(cloud), "->", len(out))
    assert unf == ref_unf and not unf and out.shape == ref.shape
    assert out.tobytes() == ref.tobytes()
    if name == "one_voxel":
        assert len(out) == 1
    if name in ("own_voxels", "n1"):
        assert len(out) == len(cloud)
    if name == "run_across_edge":
        assert len(out) == 351


def test_crop_voxel_ignoring_w_gives_the_bits_of_summing_it(ctx):
    """The local-map filter ignores the fourth sum, the cropped filter keeps it: x, y, z of the same cloud are the same bits whatever
    rides in w (the four sums are independent)."""
    xyz = room(9, 513)
    a, _ = ctx.cloud_crop_voxel(K.with_intensity(xyz, 1), FAR, 0.5)
    b, _ = ctx.cloud_crop_voxel(np.concatenate([xyz, np.full((513, 1), np.float32(np.nan))], 1), FAR, 0.5)
    assert np.ascontiguousarray(a[:, :3]).tobytes() == np.ascontiguousarray(b[:, :3]).tobytes()


# ---- the local map's filter and the grid built over its result ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_local_map_filter_matches_the_oracle(ctx, O, name):
    leaves = (ctx.cfg.leaf_corner, ctx.cfg.leaf_surf)
    clouds = [SHAPES[name](leaf) for leaf in leaves]
    T = np.eye(4)
    lm = O.LocalMap(window=50, leaf_corner=leaves[0], leaf_surf=leaves[1])
    lm.increment(clouds[0], clouds[1], T)
    ctx.map_local_reset()
    for kind in (0, 1):
        ctx.features_upload(0, kind, clouds[kind])
    sizes = ctx.map_increment_local(0, T)
    q = room(10, 300)
    for kind in (0, 1):
        want = lm.get(kind)
        got = ctx.map_local_download(kind)
        print(name, kind, len(clouds[kind]), "->", len(got))
        assert sizes[kind] == len(want) and got.tobytes() == want.tobytes()
        if len(want) >= 5:                                                   # the grid the increment rebuilt over the filtered cloud
            assert ctx.knn5(kind, q)[1].tobytes() == O.KdTree(want).knn5(q)[1].tobytes()


@pytest.mark.parametrize("name", ["n255", "n256", "n257", "n513", "max_x_last", "min_x_last"])
def test_map_set_local_grid_serves_exact_neighbours(ctx, O, name):
    cloud = SHAPES[name](0.4)
    ctx.map_set_local(0, cloud)
    q = room(11, 300)
    assert ctx.knn5(0, q)[1].tobytes() == O.KdTree(cloud).knn5(q)[1].tobytes()


# ---- mml_time_offset_search ----------------------------------------------------------------------------------------------------
def both_zeros_as_min_x(leaf):
    """+0.f and -0.f both are the minimum x (every other x is positive); which of the two the box keeps must not matter."""
    p = np.abs(room(12, 257))
    p[p[:, 0] == 0, 0] = 0.5
    p[[3, 100, 256], 0] = np.float32(0.0)
    p[[7, 200], 0] = np.float32(-0.0)
    assert np.signbit(p[:, 0]).sum() == 2 and (p[:, 0] == 0).sum() == 5
    return p


TOFS = dict({k: SHAPES[k] for k in ["n%d" % n for n in SIZES] + ["max_x_last", "min_x_last"]}, both_zeros=both_zeros_as_min_x)


@pytest.mark.parametrize("name", sorted(TOFS))
def test_time_offset_search_matches_the_oracle(ctx, O, name):
    velo = TOFS[name](0.4)
    livox = room(13, 600) + np.float32(0.05)
    g = ctx.time_offset_search(velo, livox, 50, 200)
    o = O.time_offset_search(velo, livox, 50, 200)
    assert g["nn_d2"].tobytes() == o["nn_d2"].tobytes()
    assert len(g["window_error"]) == len(o["window_error"]) == 8 and g["window_error"].tobytes() == o["window_error"].tobytes()
    assert g["best_window"] == o["best_window"] >= 0 and g["lowest_error"] == o["lowest_error"]
