"""GPU suite for the feature front end (csrc/feature.hip): every stencil and selection form at the line lengths where its dispatch decides,
against the oracle -- BIT FOR BIT, every slot, no tolerance.

The scans come from tests/feature_line_cases.py: 16 rings and 6 Livox lines of exactly chosen lengths in contexts of the default layout
whose thresholds crop nothing, so a line's length is what the test says it is.  Which form takes a line (FL.expected_form):

  call of  > 16 slots    k_stencil<0>; k_select_part narrow (161 .. 3211 points), wide (3212 .. 6411), the rest listed by k_select_list for
                         the list-mode k_select (LDS up to its capacity, global scratch beyond)
  call of <= 16 slots    k_stencil<1> + <2> (segment mode, a grid of 5056 positions per line); one direct k_select launch, LDS up to 4096 points

For every slot: xyzi, label, ring, reltime and the four label counts after extract; both down-sampled stacks after undistort (identity) +
downsample, which read the label lists the selection kernels append."""
import os

import numpy as np
import pytest

import feature_line_cases as FL

pytestmark = pytest.mark.gpu


def _context(M, B, crop=False, **over):
    if not crop:
        over.update(near_th=FL.NEAR, far_th=FL.FAR)
    return M.Context(M.default_config(B, **over))


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _where(got, want, o):
    m = min(len(got), len(want))
    g, w = got[:m].reshape(m, -1), want[:m].reshape(m, -1)
    bad = np.flatnonzero((g.view(np.uint8) != w.view(np.uint8)).any(axis=1))
    if not len(bad):
        return "%d rows for %d" % (len(got), len(want))
    i = int(bad[0])
    line = int(o["ring"][i]) + (0 if i < o["n_velo"] else FL.N_RINGS)
    lo = 0 if i < o["n_velo"] else o["n_velo"]
    at = int((o["ring"][lo:i] == o["ring"][i]).sum())      # the point's index inside its line: the fused order keeps a line's order
    return "%d rows differ, first at fused index %d = line id %d index %d: %r for %r" % (len(bad), i, line, at, g[i].tolist(), w[i].tolist())


def _check_extraction(c, s, scan, o, what):
    """slot s after extract against the oracle record of the scan it holds; returns the downloads' bytes"""
    d = c.scan_download(s)
    tag = "%s slot %d %s" % (what, s, scan.name)
    assert d["info"].n_points == len(o["xyzi"]) and d["info"].n_velo == o["n_velo"], tag
    for key in ("label", "ring"):
        assert np.array_equal(d[key], o[key]), "%s %s: %s" % (tag, key, _where(d[key], o[key], o))
    assert _same_bits(d["xyzi"], o["xyzi"]), "%s xyzi: %s" % (tag, _where(d["xyzi"], o["xyzi"], o))
    assert _same_bits(d["reltime"], o["reltime"]), "%s reltime: %s" % (tag, _where(d["reltime"], o["reltime"], o))
    i = d["info"]
    got = (i.velo_corner_num, i.velo_surf_num, i.livox_corner_num, i.livox_surf_num)
    assert got == o["counts"], (tag, got, o["counts"])
    if not scan.crop:
        assert np.array_equal(np.bincount(d["ring"][:i.n_velo], minlength=FL.N_RINGS), scan.ring_lengths or [0] * FL.N_RINGS), tag
        assert np.array_equal(np.bincount(d["ring"][i.n_velo:], minlength=FL.N_LINES), scan.line_lengths or [0] * FL.N_LINES), tag
    return (d["xyzi"].tobytes(), d["label"].tobytes(), d["ring"].tobytes(), d["reltime"].tobytes(), got)


def _run(c, O, placed, first, count, what):
    """extract(first, count) + undistort (identity) + downsample on the scans `placed` ({slot: scan}, uploaded here); every slot of the
    range against the oracle.  Returns {slot: bytes of everything downloaded}."""
    for s, scan in placed.items():
        c.scan_upload(s, scan.velo, scan.livox)
    c.extract(first, count)
    out = {}
    for s in range(first, first + count):
        out[s] = _check_extraction(c, s, placed[s], FL.oracle_fused(O, placed[s]), what)
    c.undistort(first, count, np.tile(np.eye(3).reshape(1, 9), (count, 1)), np.zeros((count, 3)))
    c.downsample(first, count)
    for s in range(first, first + count):
        o = FL.oracle_fused(O, placed[s])
        stacks = ()
        for kind, key in ((0, "corner"), (1, "surf")):
            got = c.features_download(s, kind)
            assert _same_bits(got, o[key]), "%s slot %d %s %s stack: %d voxels for %d" % (what, s, placed[s].name, key, len(got), len(o[key]))
            stacks += (got.tobytes(),)
        out[s] += stacks
    return out


_FORM_RUNS = {}   # {slot count: {scan name: bytes}} of the 12 form scans, shared by the batch and the direct test


def _form_run(M, O, count):
    """the 12 form scans through calls of `count` slots.  24: every scan in two slots, the second half in another order (other neighbours
    in the grid); 17: two calls (scans 0 .. 11 + 5 more, then the rest); 16: one call; 2, 1: one call after the other in one context."""
    if count in _FORM_RUNS:
        return _FORM_RUNS[count]
    scans = FL.form_scans()
    got = {}

    def note(placed, out):
        for s, b in out.items():
            assert got.setdefault(placed[s].name, b) == b, (count, s, placed[s].name)     # the same scan in two slots: the same bytes

    c = _context(M, count)
    try:
        if count == 24:
            order = list(range(12)) + [7, 2, 9, 4, 11, 0, 5, 10, 3, 8, 1, 6]
            calls = [{s: scans[k] for s, k in enumerate(order)}]
        elif count == 17:
            calls = [{s: scans[s % 12] for s in range(17)}, {s: scans[(11 - s) % 12] for s in range(17)}]
        elif count == 16:
            calls = [{s: scans[(s + 4) % 12] for s in range(16)}]
        else:
            calls = [{s: scans[(k + s) % 12] for s in range(count)} for k in range(0, 12, count)]
        for placed in calls:
            note(placed, _run(c, O, placed, 0, count, "extract(0, %d)" % count))
    finally:
        c.close()
    assert sorted(got) == sorted(s.name for s in scans)
    _FORM_RUNS[count] = got
    return got


def test_batch_forms(M, O):
    """Every length of the tables as a ring and as a Livox line through k_stencil<0>, both k_select_part forms and the listed k_select:
    24 slots (every scan twice), and 17, the smallest batch."""
    forms = set()
    for scan in FL.form_scans():
        forms |= {FL.expected_form(n, 24, kind) for kind, _, n in scan.lengths()}
    assert forms == {"none", "part64", "part128", "listed-lds", "listed-scratch"}
    assert _form_run(M, O, 24) == _form_run(M, O, 17)


def test_direct_forms(M, O):
    """The tables again at 1, 2 and 16 slots (stencil modes 1 + 2, the combined direct k_select): byte-identical to the batch forms'
    downloads.  Then the capacity edge of the direct form in a Velodyne-only context whose k_select holds 2048 points in LDS."""
    ref = _form_run(M, O, 24)
    for count in (16, 2, 1, 17):
        assert _form_run(M, O, count) == ref, count
    for max_velo, cap in ((16 * 1024, 2048), (FL.MAX_VELO, 4096)):
        assert FL.sel_caps(max_velo, 0)[0] == cap
        rings = [cap - 1, 161, cap, 3, cap + 1, 700, 12, 0, 160, 513, 11, 256, 37, 1000, 261, 16]
        assert FL.expected_form(cap, 1, "ring", cap, cap) == "direct-lds" and FL.expected_form(cap + 1, 1, "ring", cap, cap) == "direct-scratch"
        scan = FL.Scan("velo_only%d" % cap, rings, None, style="boundary")
        c = _context(M, 1, max_velo_points=max_velo, max_livox_points=0)
        try:
            _run(c, O, {0: scan}, 0, 1, "Velodyne-only, cap %d" % cap)
        finally:
            c.close()


def test_default_thresholds_crop_at_the_length_edges(M, O):
    """the pair with points on both sides of 2 m and 50 m in contexts with the default thresholds: 17 slots and 2"""
    a, b = FL.crop_scans()
    got = {}
    for B in (17, 2):
        c = _context(M, B, crop=True)
        try:
            placed = {s: (a, b)[s % 2] for s in range(B)}
            out = _run(c, O, placed, 0, B, "default thresholds, extract(0, %d)" % B)
            got[B] = (out[0], out[1])
            assert all(out[s] == out[s % 2] for s in range(B))
        finally:
            c.close()
    assert got[17] == got[2]


def test_all_lines_listed(M, O):
    """24 slots whose 16 rings and 6 lines are all listed: 384 ring entries for 256 workgroups, 144 Livox entries for 128 -- the list walk
    strides, the lists are as full as they get.  Then, in the same context, scans with every line eligible (nothing listed: the result
    must not depend on the lists and flags left behind), then the first set again."""
    listed, eligible = FL.listed_scans(), FL.eligible_scans()
    for s in listed:
        assert all(FL.expected_form(n, 24, kind).startswith("listed") for kind, _, n in s.lengths())
    for s in eligible:
        assert all(FL.expected_form(n, 24, kind).startswith("part") for kind, _, n in s.lengths())
    assert 24 * FL.N_RINGS > FL.SEL_ROWS[0] and 24 * FL.N_LINES > FL.SEL_ROWS[1]
    c = _context(M, 24)
    try:
        first = _run(c, O, {s: listed[(s + s // 4) % 4] for s in range(24)}, 0, 24, "all listed")
        _run(c, O, {s: eligible[s % 3] for s in range(24)}, 0, 24, "all eligible after all listed")
        again = _run(c, O, {s: listed[(s + s // 4) % 4] for s in range(24)}, 0, 24, "all listed again")
        assert first == again
    finally:
        c.close()


def test_hand_over_order(M, O):
    """narrow / wide / listed alternating over consecutive line ids (all three rotations): the narrow form resets sel_done, the wide form
    reads it, k_select_list lists what is left -- across the 4-line and 2-line groupings of a workgroup, line ids 20 and 21 included"""
    scans = FL.handover_scans()
    for rot, s in enumerate(scans):
        kinds = [("n", "w", "l")[(i + rot) % 3] for i in range(22)]
        want = {"n": "part64", "w": "part128"}
        for (kind, _, n), k in zip(s.lengths(), kinds):
            f = FL.expected_form(n, 24, kind)
            assert (f == want[k]) if k in want else f.startswith("listed"), (s.name, kind, n)
    c = _context(M, 24)
    try:
        out = _run(c, O, {s: scans[(s + s // 3) % 3] for s in range(24)}, 0, 24, "hand-over")
        c2 = _context(M, 2)
        try:
            for k in range(3):
                direct = _run(c2, O, {0: scans[k], 1: scans[(k + 1) % 3]}, 0, 2, "hand-over scans, direct")
                slot = next(s for s in range(24) if (s + s // 3) % 3 == k)
                assert direct[0] == out[slot]
        finally:
            c2.close()
    finally:
        c.close()


def test_segment_boundaries_at_chosen_line_indices(M, O):
    """Livox lines of 600 and 3300 points whose first segment ends at line index 63, 64, 65, 255, 256, 257, 261 and n - 6, and a line with
    two segment boundaries inside one 64-index round (the general translation path): 24 slots and 2, the one-pass bucketing and the
    three-pass form (MML_ASSIGN_ONEPASS=0, read when the context is created) -- byte-equal downloads."""
    scans, _ = FL.segment_scans()
    got = {}
    for form in ("1", "0"):
        for B in (24, 2):
            os.environ["MML_ASSIGN_ONEPASS"] = form
            try:
                c = _context(M, B)
            finally:
                del os.environ["MML_ASSIGN_ONEPASS"]
            try:
                res = {}
                for k in range(0, 3 if B == 2 else 1):
                    placed = {s: scans[(s + k + s // 3) % 3] for s in range(B)}
                    for s, b in _run(c, O, placed, 0, B, "onepass=%s extract(0, %d)" % (form, B)).items():
                        assert res.setdefault(placed[s].name, b) == b
                got[form, B] = res
            finally:
                c.close()
    assert got["1", 24] == got["1", 2] == got["0", 24] == got["0", 2] and len(got["1", 24]) == 3


def test_slot_independence_and_first_slot(M, O):
    """A slot's downloads do not change when its neighbours' scans are replaced by scans of other forms, nor when the call does not start
    at slot 0 (extract(5, 18) in a 24-slot context)."""
    forms, others = FL.form_scans(), FL.handover_scans() + FL.listed_scans() + FL.eligible_scans()
    keep = (6, 7, 12, 21)
    c = _context(M, 24)
    try:
        placed = {s: forms[s % 12] for s in range(24)}
        base = _run(c, O, placed, 0, 24, "independence, first set")
        placed2 = {s: (placed[s] if s in keep else others[s % len(others)]) for s in range(24)}
        swapped = _run(c, O, placed2, 0, 24, "independence, neighbours replaced")
        for s in keep:
            assert swapped[s] == base[s], s
        part = _run(c, O, {s: placed2[s] for s in range(5, 23)}, 5, 18, "extract(5, 18)")
        for s in range(5, 23):
            assert part[s] == swapped[s], s
        # the slots outside the range still hold the fused clouds of the call before
        for s in (0, 4, 23):
            assert c.scan_info(s).n_points == len(FL.oracle_fused(O, placed2[s])["xyzi"])
    finally:
        c.close()
