"""GPU suite for the per-slot voxel filter: every form of k_voxel (csrc/undistort_voxel.hip) and the global-sort redo
(csrc/map_upkeep.hip) at the edges of their labelled counts, in both key layouts, against tests/voxel_cases.py's plain restatement
of pcl::VoxelGrid -- BIT FOR BIT, every slot, no tolerance.

The labelled clouds come in through mml_cloud_upload (label in normal_z; k_crop builds the label lists k_voxel reads), so a test
chooses the number of labelled points of a (slot, kind), their voxel structure and their fused indices.  Which form takes a list:

  call of <= 16 slots    k_voxel<1024> for both kinds: corner lists up to 2048, surf lists up to 8192 points
  call of  > 16 slots    k_voxel<256> corners (2048), k_voxel<512> surf lists up to 4096, k_voxel<1024, LIST> the longer ones (8192)
  NT > 65536             k_voxel<1024> for both kinds, 8192 points each, the wide key layout (voxel 31 | fused index 20 | place 13)
  beyond the capacity    marked by k_voxel, redone by mml_downsample_big (one global sort); NT > 2^20: refused

Each form has a 1-, 2-, 4- and 8-keys-per-lane branch (T, 2 T, 4 T, 8 T keys for T threads); the tables hold T - 1, T, T + 1 of each.
"edge" lists put an r-point voxel in the last place of the centroid pass's first chunk (r = 65, 66 on either side of the 64 staged
points beyond a chunk, r = T + 70 across a whole chunk).  All points in one voxel: the fused index is part of the sorted bits, so only
the one-point list takes the sort's "nothing to sort" exit; 300 and 2048 points in one voxel sort on the fused index alone."""
import numpy as np
import pytest

import voxel_cases as V

pytestmark = pytest.mark.gpu

NVP, NLP = 9000, 600      # max_velo_points, max_livox_points of the small contexts
SENTINEL = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]], np.float32)


def _upload(c, slot, case, nvp=NVP):
    c.cloud_upload(slot, case.records(nvp), case.n_velo)


def _poison(c, slots):
    """stacks no down-sampling would leave: a call that skips a slot shows"""
    for s in slots:
        for kind in (0, 1):
            c.features_upload(s, kind, SENTINEL + kind)


def _is_poison(c, s):
    return all(c.features_download(s, kind).tobytes() == (SENTINEL + kind).tobytes() for kind in (0, 1))


def _check(c, slot, case, what=""):
    """both stacks of the slot against the reference; returns their bytes"""
    info = c.scan_info(slot)
    assert (info.n_points, info.n_velo, info.fused_corner_num, info.fused_surf_num) == (case.n, case.n_velo) + case.counts, (what, slot, case.name)
    out = []
    for kind in (0, 1):
        want, got = case.expected(kind), c.features_download(slot, kind)
        if got.tobytes() != want.tobytes():
            m = min(len(got), len(want))
            bad = np.flatnonzero((got[:m].view(np.uint32) != want[:m].view(np.uint32)).any(axis=1))
            first = int(bad[0]) if len(bad) else m
            pytest.fail("%s slot %d %s kind %d: %d voxels for %d; %d rows differ, first at %d: %r for %r" % (
                what, slot, case.name, kind, len(got), len(want), len(bad), first, got[first:first + 1].tolist(), want[first:first + 1].tolist()))
        out.append(got.tobytes())
    return out


def _rotated(cases):
    """the lists beyond a form's capacity (first and last of a table) into the middle of the batch"""
    k = len(cases) // 2
    return cases[k:] + cases[:k]


def test_small_batch_form(M):
    cases = _rotated(V.small_batch_cases())
    c = M.Context(max_scans=16, max_velo_points=NVP, max_livox_points=NLP, max_features=16384)
    try:
        for r0 in range(0, len(cases), 16):
            group = cases[r0:r0 + 16]
            for s, case in enumerate(group):
                _upload(c, s, case)
            _poison(c, range(16))
            c.downsample(0, len(group))
            for s, case in enumerate(group):
                _check(c, s, case, "downsample(0, %d)" % len(group))
            assert all(_is_poison(c, s) for s in range(len(group), 16))
        # one slot per call
        for case in cases[:3]:
            _upload(c, 5, case)
            _poison(c, (4, 5, 6))
            c.downsample(5, 1)
            _check(c, 5, case, "downsample(5, 1)")
            assert _is_poison(c, 4) and _is_poison(c, 6)
        _upload(c, 0, cases[4])
        c.downsample(0, 1)
        _check(c, 0, cases[4], "downsample(0, 1)")
    finally:
        c.close()


def test_large_batch_forms(M):
    cases = _rotated(V.large_batch_cases())
    B, first = 48, 5
    assert 16 < len(cases) <= B - first - 2
    quiet = V.quiet_cases(3)
    c = M.Context(max_scans=B, max_velo_points=NVP, max_livox_points=NLP, max_features=16384)
    try:
        outside = [s for s in range(B) if not first <= s < first + len(cases)]
        for s in outside:
            _upload(c, s, quiet[s % 3])       # (labelled clouds: a launch that reached them would replace the stacks)
        for s, case in enumerate(cases):
            _upload(c, first + s, case)
        _poison(c, range(B))
        c.downsample(first, len(cases))
        for s, case in enumerate(cases):
            _check(c, first + s, case, "downsample(%d, %d)" % (first, len(cases)))
        assert all(_is_poison(c, s) for s in outside)
    finally:
        c.close()


def test_form_independence_and_ranges(M):
    cases, quiet = V.independence_cases(), V.quiet_cases(20)
    c = M.Context(max_scans=44, max_velo_points=NVP, max_livox_points=NLP, max_features=16384)
    try:
        for s, case in enumerate(cases):
            _upload(c, s, case)
        for s, case in enumerate(quiet):
            _upload(c, 24 + s, case)
        got = {}
        for first, count in ((0, 16), (0, 17), (3, 20)):
            _poison(c, range(44))
            c.downsample(first, count)
            got[first, count] = {s: _check(c, s, cases[s], "downsample(%d, %d)" % (first, count)) for s in range(first, first + count)}
            assert all(_is_poison(c, s) for s in range(44) if not first <= s < first + count)
        for s in range(3, 16):
            assert got[0, 16][s] == got[0, 17][s] == got[3, 20][s], s
        assert got[0, 17][16] == got[3, 20][16]
        # after a call whose listed launch had work: a range without a long list, elsewhere ...
        _poison(c, range(44))
        c.downsample(24, 20)
        for s, case in enumerate(quiet):
            _check(c, 24 + s, case, "downsample(24, 20)")
        assert all(_is_poison(c, s) for s in range(24))
        # ... and the same range as the call that had long lists, its slots now holding short ones
        for s in range(3, 23):
            _upload(c, s, quiet[s - 3])
        _poison(c, range(44))
        c.downsample(3, 20)
        for s in range(3, 23):
            _check(c, s, quiet[s - 3], "downsample(3, 20) again")
        assert all(_is_poison(c, s) for s in (0, 1, 2, 23, 24, 43))
    finally:
        c.close()


def test_listed_form_longer_than_its_grid(M):
    """270 surf lists of 4097 points in one call: the listed launch has 256 workgroups, 14 of them take a second list"""
    big, small = V.long_list_cases()
    B = 300
    cases = [small[(s // 10) % 4] if s % 10 == 3 else big[s % 4] for s in range(B)]
    assert sum(case.counts[1] > 4096 for case in cases) >= 260
    rec = {case.name: case.records(4300) for case in big + small}
    c = M.Context(max_scans=B, max_velo_points=4300, max_livox_points=64, max_features=8192)
    try:
        for s, case in enumerate(cases):
            c.cloud_upload(s, rec[case.name], case.n_velo)
        c.downsample(0, B)
        for s, case in enumerate(cases):
            _check(c, s, case, "downsample(0, 300)")
    finally:
        c.close()


def test_wide_key_layout(M):
    cases = V.wide_cases()
    c = M.Context(max_scans=len(cases), max_velo_points=65600, max_livox_points=64, max_features=16384)
    try:
        for s, case in enumerate(cases):
            assert case.n == 65650 and case.n_velo + 64 > 65536      # the Livox part lies beyond position 65536
            _upload(c, s, case, 65600)
        _poison(c, range(len(cases)))
        c.downsample(0, len(cases))
        for s, case in enumerate(cases):
            _check(c, s, case, "wide")
    finally:
        c.close()


def test_wide_key_layout_at_2_pow_20(M):
    c = M.Context(max_scans=1, max_velo_points=(1 << 20) - 64, max_livox_points=64, max_features=16384)
    try:
        for case in V.full_cases():
            xyz, label = case.cloud()
            assert len(xyz) == 1 << 20 and label[-1] != 0             # fused index 2^20 - 1 is labelled
            c.cloud_upload(0, V.records(xyz, label, case.n_velo, full=True), case.n_velo)
            _poison(c, (0,))
            c.downsample(0, 1)
            _check(c, 0, case, "2^20 points")
    finally:
        c.close()


def test_capacity_is_reported_not_truncated(M):
    cases = V.capacity_cases()
    c = M.Context(max_scans=4, max_velo_points=NVP, max_livox_points=NLP, max_features=1000)
    try:
        for s, case in enumerate(cases):
            _upload(c, s, case)
        c.downsample(0, 4)
        for s, case in enumerate(cases):
            if len(case.expected(0)) <= 1000:
                assert len(case.expected(0)) == len(case.expected(1)) == 1000
                _check(c, s, case, "max_features = 1000")
                continue
            for kind in (0, 1):
                if len(case.expected(kind)) > 1000:
                    assert len(case.expected(kind)) == 1001
                    with pytest.raises(M.MmlError) as e:
                        c.features_download(s, kind)
                    assert e.value.code == M.MML_ERR_CAPACITY, (s, kind)
                else:
                    assert c.features_download(s, kind).tobytes() == case.expected(kind).tobytes()
    finally:
        c.close()
    # scans beyond 2^20 points: the global-sort filter is the only path and refuses them
    c = M.Context(max_scans=2, max_velo_points=1 << 20, max_livox_points=64, max_features=1000)
    try:
        case = V.quiet_cases(1)[0]
        _upload(c, 0, case, 1 << 20)
        c.cloud_upload(1, case.records()[:, :] * np.float32([1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1]), case.n_velo)   # the same cloud, no labels
        _poison(c, (0, 1))
        with pytest.raises(M.MmlError) as e:
            c.downsample(0, 1)
        assert e.value.code == M.MML_ERR_CAPACITY
        assert _is_poison(c, 0)                                        # nothing was written for the refused slot
        c.downsample(1, 1)
        assert len(c.features_download(1, 0)) == 0 and len(c.features_download(1, 1)) == 0
    finally:
        c.close()
