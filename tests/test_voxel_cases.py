"""CPU checks of tests/voxel_cases.py: the plain VoxelGrid restatement against the oracle's independent one, bit for bit, on every
list of every case table and at both leaf sizes; and the properties that make the cases worth running on the device -- the labelled
counts, where the long run of a chunk-edge list starts in the sorted order, one voxel / one voxel per point, which lists overflow the
grid, which index bits differ, and that the order of a voxel's float sum shows in the bits."""
import numpy as np
import pytest

import voxel_cases as V

CASES = V.all_cases()
LISTS = {}
for _c in CASES:
    for _k in (0, 1):
        LISTS.setdefault((V.spec_name(_c.specs[_k]), _k), (_c, _k))
LIST_IDS = ["%s-%s" % (n, "corner" if k == 0 else "surf") for n, k in LISTS]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_reference_equals_the_oracle_bit_for_bit(O, case):
    for kind in (0, 1):
        pts = case.lists[kind]
        for leaf in V.LEAF:
            ref = V.voxel_ref(pts, leaf)
            assert ref.dtype == np.float32 and ref.tobytes() == O.voxel_downsample(pts, leaf).tobytes(), (case.name, kind, leaf)
        assert case.expected(kind).tobytes() == V.voxel_ref(pts, V.LEAF[kind]).tobytes()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cloud_holds_the_intended_lists_in_fused_order(case):
    xyz, label = case.cloud()
    assert len(xyz) == case.n and xyz.dtype == np.float32
    for kind in (0, 1):
        assert int((label == kind + 1).sum()) == case.counts[kind] == V.spec_n(case.specs[kind])
        assert xyz[label == kind + 1].tobytes() == case.lists[kind].tobytes()
    lab = np.flatnonzero(label)
    if case.layout == "tail":       # the labelled points hold the highest fused indices, the Livox part among them
        assert len(lab) == 0 or (lab[0] == case.n - len(lab) and lab[-1] == case.n - 1 and lab[0] < case.n_velo)
    elif len(lab) > 64:             # interleaved with the label-0 points and with each other
        assert len(set(label[lab[0]:lab[-1] + 1])) == len(set(label))
    if case.full:
        assert case.n == 1 << 20 and case.n_velo == (1 << 20) - 64
    else:
        assert 0 < case.n_velo < case.n
    rec = case.records() if case.n <= 70000 else V.records(xyz[-8:], label[-8:], 3)
    assert rec.shape[1] == 12 and rec.dtype == np.float32 and rec[:, 3].max() == 0 and rec[:, 7].max() == 0 and rec[:, 9:].max() == 0
    if case.n <= 70000:
        assert np.array_equal(rec[:, 6], label) and rec[:, :3].tobytes() == xyz.tobytes()


def _reversed_sum_differs(pts):
    return V.seq_sum(pts).tobytes() != V.seq_sum(pts[::-1]).tobytes()


@pytest.mark.parametrize("key", list(LISTS), ids=LIST_IDS)
def test_list_has_the_structure_its_spec_names(key):
    case, kind = LISTS[key]
    spec, pts, leaf = case.specs[kind], case.lists[kind], V.LEAF[kind]
    n = V.spec_n(spec)
    assert len(pts) == n
    if n == 0:
        return
    assert V.grid_overflows(pts, leaf) == (spec["kind"] == "overflow")
    if spec["kind"] == "overflow":
        assert case.expected(kind).tobytes() == pts.tobytes()
        return
    order, starts, lengths = V.voxel_runs(pts, leaf)
    idx = V.voxel_index(pts, leaf)
    if n > 64 and spec["kind"] != "one":   # the fused order is not the voxel order
        assert not np.array_equal(order, np.arange(n))
    if spec["kind"] == "count":
        assert lengths.max() <= 3 and (n < 8 or (lengths.min() == 1 and lengths.max() > 1))
    elif spec["kind"] == "own":
        assert len(starts) == n == len(case.expected(kind))
    elif spec["kind"] == "one":
        assert len(starts) == 1 == len(case.expected(kind))
        assert n < 3 or _reversed_sum_differs(pts[order])
    elif spec["kind"] == "voxels":
        assert len(starts) == spec["voxels"] == len(case.expected(kind))
    elif spec["kind"] == "edge":
        T, r = spec["T"], spec["r"]
        assert np.array_equal(lengths, [1] * (T - 1) + [r] + [1] * spec["extra"])
        assert starts[T - 1] == T - 1 and lengths[T - 1] == r       # the r-point voxel starts in the last place of the first chunk
        # (two floats add to the same sum either way round: r = 2 tests where the run lies, not the order it is summed in)
        assert r < 3 or _reversed_sum_differs(pts[order[T - 1:T - 1 + r]])
        # the order of the points inside the run is the fused order, which is not the order of x
        assert r < 3 or not np.array_equal(np.argsort(pts[order[T - 1:T - 1 + r], 0]), np.arange(r))
    elif spec["kind"] == "digit16":
        u = np.unique(idx)
        assert len(u) == 2 and (u[0] ^ u[1]) & 0xffff == 0 and (u[0] ^ u[1]) >> 16 != 0
        assert all(_reversed_sum_differs(pts[order[s:s + m]]) for s, m in zip(starts, lengths))
    elif spec["kind"] == "digit24":
        _, _, div_b, _ = V._grid(pts, leaf)
        assert (1 << 30) < int(np.prod(div_b)) < (1 << 31)
        assert int(np.bitwise_or.reduce(idx) ^ np.bitwise_and.reduce(idx)) >> 24 != 0 and int(idx.max()) >> 30 == 1
        assert lengths.max() == 2
    elif spec["kind"] == "arith":
        inv = np.float32(1) / np.float32(leaf)
        on_lattice = (np.float32(leaf) * np.round(pts * inv) == pts).all(axis=1)
        assert on_lattice.sum() > n // 3 and (~on_lattice).sum() > n // 8
        assert (pts < 0).any() and np.signbit(pts[pts == 0]).any() and not np.signbit(pts[pts == 0]).all()
        assert len(np.unique(pts, axis=0)) < n - n // 8 and lengths.max() > 2


def test_tables_reach_every_form_at_its_count_edges():
    """the counts the kernel's branches need: T - 1, T, T + 1 of each keys-per-lane branch of each form, the capacities, one beyond"""
    def counts(cases, kind):
        return {c.counts[kind] for c in cases}
    small, large = V.small_batch_cases(), V.large_batch_cases()
    base = {0, 1, 2, 63, 64, 65}
    assert base | {255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049} <= counts(large, 0)
    assert base | {511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193} <= counts(large, 1)
    assert base | {1023, 1024, 1025, 2047, 2048, 2049} <= counts(small, 0)
    assert base | {2049, 4096, 4097, 8192, 8193} <= counts(small, 1)
    edges = lambda cases, kind: {(c.specs[kind]["T"], c.specs[kind]["r"]) for c in cases if c.specs[kind]["kind"] == "edge"}
    assert {(256, r) for r in (2, 64, 65, 66, 326)} <= edges(large, 0)
    assert {(512, r) for r in (2, 64, 65, 66, 582)} <= edges(large, 1)
    assert {(1024, r) for r in (2, 64, 65, 66)} <= edges(small, 0) and {(1024, r) for r in (2, 64, 65, 66, 1094)} <= edges(small, 1)
    assert {c.counts for c in V.wide_cases()} >= {(8191, 8192), (8192, 8191)} and 8193 in counts(V.wide_cases(), 0) | counts(V.wide_cases(), 1)
    for c in small + large + V.independence_cases():
        assert c.n_velo < 9000 and c.n - c.n_velo <= 600
    assert len(large) > 16 and len(V.independence_cases()) == 23
    big, _ = V.long_list_cases()
    assert all(c.counts[1] == 4097 and c.n_velo < 4300 for c in big)
