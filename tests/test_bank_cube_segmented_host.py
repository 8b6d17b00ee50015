"""The segmented cube-store calls without a device: mml_map_bank_global_increment_segmented, mml_map_bank_global_append_segmented and
mml_debug_bank_global_increment_budget are declared and exported and refuse a NULL context; BatchLidarOdometry hands the choice
on and refuses any other word; the chunk rule of the header (greedy, call order, a bank over the budget alone, the cap on the banks
of a chunk) restated in numpy gives the chunks written down by hand; and the sort key's layout -- segment << 53 | cube << 40 |
voxel index -- packs and unpacks its largest fields without loss."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["mml_map_bank_global_increment_segmented", "mml_map_bank_global_append_segmented", "mml_debug_bank_global_increment_budget"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmloam_hip.h")).read(), flags=re.S)


def test_names_declared_and_exported(M):
    src = _header()
    assert re.search(r"\bint\s+mml_map_bank_global_increment_segmented\s*\(\s*mml_ctx\s*\*\s*ctx,\s*int n,\s*const int\s*\*\s*banks,"
                     r"\s*const double\s*\*\s*T_wl,\s*int\s*\*\s*n_corner,\s*int\s*\*\s*n_surf\)", src)
    assert re.search(r"\bint\s+mml_map_bank_global_append_segmented\s*\(\s*mml_ctx\s*\*\s*ctx,\s*int n,\s*const int\s*\*\s*banks,"
                     r"\s*const int\s*\*\s*slots,\s*const double\s*\*\s*T_wl\)", src)
    assert re.search(r"\bint\s+mml_debug_bank_global_increment_budget\s*\(\s*mml_ctx\s*\*\s*ctx,\s*long points\)", src)
    for n in NAMES:
        assert hasattr(M.lib(), n), "libmmloam_hip.so does not export %s" % n
    for n in ("bank_global_increment", "bank_global_append", "bank_global_increment_budget"):
        assert hasattr(M.Context, n)


def test_null_context_is_an_argument_error(M):
    L, p = M.lib(), M._p
    one = np.zeros(1, np.int32)
    T = np.eye(4).reshape(1, 16)
    assert L.mml_map_bank_global_increment_segmented(None, 1, p(one), p(T), None, None) == M.MML_ERR_INVALID
    assert L.mml_map_bank_global_increment_segmented(None, 0, None, None, None, None) == M.MML_ERR_INVALID
    assert L.mml_map_bank_global_append_segmented(None, 1, p(one), p(one), p(T)) == M.MML_ERR_INVALID
    assert L.mml_debug_bank_global_increment_budget(None, C.c_long(100)) == M.MML_ERR_INVALID


class _Stub:
    """Records how the two cube calls of a round were made; everything else BatchLidarOdometry(global_map=True) needs for a first
    round (empty maps: no Estimate)."""

    def __init__(self):
        self.calls = []

    def map_banks(self, n):
        pass

    def bind_banks(self, first, banks):
        pass

    def scan_info(self, slot):
        import types
        return types.SimpleNamespace(fused_corner_num=200)

    def downsample(self, first, count):
        pass

    def features_count(self, slot, kind):
        return 500

    def bank_increment(self, *a, **kw):
        return np.full(len(a[0]), 100, np.int32), np.full(len(a[0]), 1000, np.int32)

    def bank_global_append(self, *a, **kw):
        self.calls.append(("append", len(a), dict(kw)))

    def bank_global_increment(self, *a, **kw):
        self.calls.append(("increment", len(a), dict(kw)))
        return np.full(len(a[0]), 10, np.int32), np.full(len(a[0]), 20, np.int32)


def test_batch_odometry_hands_the_choice_on():
    odometry = importlib.import_module("multi-modal-loam_amd.odometry")
    P, Q = np.zeros((2, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (2, 1))
    for how, want in (({}, {}), (dict(global_increment="loop"), {}), (dict(global_increment="segmented"), dict(segmented=True))):
        ctx = _Stub()
        bat = odometry.BatchLidarOdometry(ctx, 2, global_map=True, map_skip_frame=1, **how)
        bat.estimate_lidar_pose([0, 1], P, Q)
        # "loop": the positional arguments of before and nothing else
        assert ctx.calls == [("append", 3, want), ("increment", 2, want)]
    with pytest.raises(ValueError):
        odometry.BatchLidarOdometry(_Stub(), 2, global_increment="x")
    with pytest.raises(ValueError):
        odometry.BatchLidarOdometry(_Stub(), 2, global_map=True, global_increment="both")


def _chunks(pts, budget, max_banks):
    """The rule of include/mmloam_hip.h: greedy, in call order; a chunk holds at most `budget` points and at most `max_banks`
    banks; a bank over the budget is a chunk of its own.  Returns the chunks as lists of positions in the call."""
    pts = np.asarray(pts, dtype=np.int64)
    out, cur, run = [], [], 0
    for i, p in enumerate(pts):
        if cur and (run + p > budget or len(cur) >= max_banks):
            out.append(cur)
            cur, run = [], 0
        cur.append(i)
        run += int(p)
    if cur:
        out.append(cur)
    return out


def test_chunk_rule_on_hand_written_lists():
    # all fit: one chunk
    assert _chunks([10, 20, 30], 100, 128) == [[0, 1, 2]]
    # greedy, call order: 60 + 30 fit, 20 more do not; a later small bank does not move forward into an earlier chunk
    assert _chunks([60, 30, 20, 90, 5], 100, 128) == [[0, 1], [2], [3, 4]]
    # a bank over the budget is alone, wherever it stands; empty banks cost nothing
    assert _chunks([0, 250, 0, 0, 40, 300], 100, 128) == [[0], [1], [2, 3, 4], [5]]
    # the cap on the banks of a chunk cuts before the budget does
    assert _chunks([1, 1, 1, 1, 1, 1, 1], 100, 3) == [[0, 1, 2], [3, 4, 5], [6]]
    # every bank lies in exactly one chunk, in order
    rng = np.random.default_rng(3)
    pts = rng.integers(0, 200, 50)
    ch = _chunks(pts, 300, 4)
    assert [i for c in ch for i in c] == list(range(50))
    assert all(len(c) <= 4 and (len(c) == 1 or pts[c].sum() <= 300) for c in ch)


def test_header_states_the_defaults():
    src = _header()
    assert re.search(r"#define\s+MML_BANK_GLOBAL_INCREMENT_BUDGET\s+\(1 << 22\)", src)
    m = re.search(r"#define\s+MML_BANK_GLOBAL_CHUNK_BANKS\s+(\d+)", src)
    assert m and 2 * int(m.group(1)) <= 2048            # the segments of a chunk fit the key's 11 segment bits


def _pack(seg, cube, vox):
    return (seg << 53) | (cube << 40) | vox


def _unpack(key):
    return key >> 53, (key >> 40) & 0x1FFF, key & ((1 << 40) - 1)


def test_key_layout_round_trips():
    vox = (1 << 40) - 1
    key = _pack(2047, 4850, vox)
    assert key < (1 << 64) and _unpack(key) == (2047, 4850, vox)
    assert _unpack(_pack(0, 0, 0)) == (0, 0, 0) and _unpack(_pack(1, 0, 0)) == (1, 0, 0)
    assert 4850 < (1 << 13) and 53 + 11 == 64
    # the order the sort sees: segment, then cube, then voxel
    keys = [_pack(s, c, v) for s in (0, 5, 2047) for c in (0, 17, 4850) for v in (0, 3, vox)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    # as uint64, the type the device sorts
    k = np.array(keys, dtype=np.uint64)
    assert np.array_equal(k >> np.uint64(53), np.repeat([0, 5, 2047], 9).astype(np.uint64))
    assert np.array_equal((k >> np.uint64(40)) & np.uint64(0x1FFF), np.tile(np.repeat([0, 17, 4850], 3), 3).astype(np.uint64))
