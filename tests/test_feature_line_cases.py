"""CPU checks of tests/feature_line_cases.py: every scan holds the line lengths it was built for (the oracle's fused per-ring counts),
expected_form names the intended form at every table length and slot count, the partition sizes at the deciding lengths are what the
tables claim, the lines keep the selection busy (flags 2, 100 / 101, 150; labels on both sides of partition boundaries; marks across
them), the explicit Livox placements put the segment boundaries where they are meant to be, and -- for the lengths up to 700 -- the
oracle's detectFeaturePoints equals the pure-Python second restatement, flags included."""
import numpy as np
import pytest

import feature_line_cases as FL
import second_opinion

FORM_SCANS = FL.form_scans()
SEG_SCANS, SEG_SPECS = FL.segment_scans()
ALL_SCANS = FORM_SCANS + FL.listed_scans() + FL.eligible_scans() + FL.handover_scans() + SEG_SCANS
IDS = [s.name for s in ALL_SCANS]


def test_tables_and_constants():
    assert FL.sel_caps() == (FL.SEL_CAP, FL.SEL_CAP_VELO) == (4096, 2048) and FL.NOMINAL == 5056
    assert FL.sel_caps(16 * 1024, 0) == (2048, 2048)               # the Velodyne-only context of the direct-form test
    assert FL.TABLES["tiles"] == [250, 251, 255, 256, 257, 261, 262, 266, 267, 506, 507, 511, 512, 513, 517, 518, 522, 523]
    assert FL.TABLES["segment_grid"] == [5055, 5056, 5057, 5313] and FL.TABLES["direct_caps"] == [2047, 2048, 2049, 4095, 4096, 4097]
    assert len(FL.ALL_LENGTHS) == 58
    # every length of the tables is a ring of one form scan and a Livox line of another
    rings = [n for s in FORM_SCANS for n in s.ring_lengths]
    lines = [n for s in FORM_SCANS for n in s.line_lengths]
    for n in FL.ALL_LENGTHS:
        assert n in rings and n in lines, n
    for s in FORM_SCANS:
        assert len(set(FL.expected_form(n, 24, k) for k, _, n in s.lengths())) >= 3, s.name      # a scan mixes the forms


def test_partition_sizes_at_the_deciding_lengths():
    for n, (lo, hi, n_hi) in FL.PARTITION_CLAIMS.items():
        size = FL.partition_sizes(n)
        assert size.sum() == n - 11 and size.min() == lo and size.max() == hi, n
        if hi > lo:
            assert (size == hi).sum() == n_hi == 1, n
    assert FL.partition_starts(161)[0] == 5 and FL.partition_starts(161)[-1] == 161 - 6
    # the partitions straddle the 64-point windows: at 3211 points partition j starts at 5 + 64 j
    assert np.array_equal(FL.partition_starts(3211) % 64, np.full(51, 5))


def test_expected_form_at_every_table_length():
    want24 = {160: "listed-lds", 161: "part64", 3211: "part64", 3212: "part128", 6411: "part128", 6412: "listed-scratch", 1: "listed-lds",
              0: "none", 2049: "part64", 4097: "part128", 6500: "listed-scratch"}
    for n in FL.ALL_LENGTHS:
        for kind in ("ring", "livox"):
            for count in (17, 24):
                f = FL.expected_form(n, count, kind)
                if n == 0:
                    assert f == "none"
                elif n <= 160:
                    assert f == "listed-lds"
                elif n <= 3211:
                    assert f == "part64"
                elif n <= 6411:
                    assert f == "part128"
                else:
                    assert f == "listed-scratch"
                if n in want24:
                    assert f == want24[n]
            for count in (1, 16):
                f = FL.expected_form(n, count, kind)
                assert f == ("none" if n == 0 else "direct-lds" if n <= 4096 else "direct-scratch"), (n, count)
    # the listed forms' own capacity edges (reachable only with other capacities: a line of 161 .. 6411 points is never listed)
    assert FL.expected_form(7000, 24, "ring") == FL.expected_form(7000, 24, "livox") == "listed-scratch"
    assert FL.expected_form(160, 24, "ring", 128, 128) == "listed-scratch" and FL.expected_form(2049, 1, "ring", 2048, 2048) == "direct-scratch"
    assert FL.expected_form(2048, 1, "ring", 2048, 2048) == "direct-lds"


@pytest.mark.parametrize("scan", ALL_SCANS + FL.crop_scans(), ids=IDS + ["crop0", "crop1"])
def test_scans_hold_the_intended_lengths(O, scan):
    if scan.velo is not None:
        assert scan.velo.shape == (sum(scan.ring_lengths), 4) and scan.velo.dtype == np.float32
        ev = O.extract_velo(scan.velo, near=FL.NEAR, far=FL.FAR)
        assert np.array_equal(np.bincount(ev["ring"], minlength=16), scan.ring_lengths)
        for r in (0, 7, 15):      # ring r of the fused cloud is rings[r], in order (the reference writes intensity 0 for Velodyne points)
            assert ev["xyzi"][ev["ring"] == r][:, :3].tobytes() == scan.rings[r][:, :3].tobytes()
    if scan.livox is not None:
        assert len(scan.livox) <= FL.MAX_LIVOX
        el = O.extract_livox(scan.livox, near=FL.NEAR, far=FL.FAR)
        assert np.array_equal(np.bincount(el["ring"], minlength=6), scan.line_lengths)
        for j in range(6):
            assert el["xyzi"][el["ring"] == j].tobytes() == scan.lines[j].tobytes()
    if scan.crop:                 # the default thresholds drop points of these scans on both sides
        o = FL.oracle_fused(O, scan)
        d2 = (np.concatenate([scan.velo[:, :3]] + [l[:, :3] for l in scan.lines]).astype(np.float64) ** 2).sum(1)
        assert (d2 < 4.0).sum() > 100 and (d2 > 2500.0).sum() > 100 and len(o["xyzi"]) < len(d2) - 200
        assert ((d2 > 3.6) & (d2 < 4.0)).sum() > 20 and ((d2 > 4.0) & (d2 < 4.5)).sum() > 20


def _activity(O, lines):
    """flag counts, partition boundaries with a label within 3 points on each side, boundaries that a run of marks crosses"""
    tot = dict(f2=0, f100=0, f150=0, both_sides=0, mark_cross=0, lines=0)
    for pts in lines:
        n = len(pts)
        if n < 12:
            continue
        sharp, flat, flags = O.detect_feature_points(pts)
        tot["lines"] += 1
        tot["f2"] += int((flags == 2).sum())
        tot["f100"] += int(((flags == 100) | (flags == 101)).sum())
        tot["f150"] += int((flags == 150).sum())
        lab = np.zeros(n, bool)
        lab[sharp] = True
        lab[flat] = True
        if n < 161:
            continue
        for b in FL.partition_starts(n)[1:-1]:
            tot["both_sides"] += int(lab[b - 3:b].any() and lab[b:b + 3].any())
            # a mark (flag 1) next to a picked or marked point on the other side of the boundary
            tot["mark_cross"] += int((flags[b - 1] == 1 and flags[b] in (1, 2, 3)) or (flags[b] == 1 and flags[b - 1] in (1, 2, 3)))
    return tot


def test_the_lines_exercise_the_selection(O):
    """What the oracle gives (asserted floors: at most half of it):
         form scans, Livox lines   flag 2: 20282   100 / 101: 1933   150: 878    boundaries labelled on both sides: 706    marks across: 1706
         form scans, rings         flag 2: 36839   100 / 101: 3181   150: 1333   boundaries labelled on both sides: 1662   marks across: 3427
         hand-over + listed + eligible + segment scans, all lines:
                                   flag 2: 51410   100 / 101: 5611   150: 2597   boundaries labelled on both sides: 1939   marks across: 5184"""
    got = {}
    got["livox"] = _activity(O, [l for s in FORM_SCANS for l in s.lines])
    got["rings"] = _activity(O, [r for s in FORM_SCANS for r in s.rings])
    got["other"] = _activity(O, [l for s in ALL_SCANS[12:] for l in s.lines + s.rings])
    floors = dict(livox=dict(f2=10000, f100=960, f150=430, both_sides=350, mark_cross=850),
                  rings=dict(f2=18000, f100=1590, f150=660, both_sides=830, mark_cross=1700),
                  other=dict(f2=25000, f100=2800, f150=1290, both_sides=960, mark_cross=2590))
    for table, fl in floors.items():
        for key, floor in fl.items():
            assert got[table][key] >= floor, (table, key, got[table][key])
        assert got[table]["both_sides"] >= 10 and got[table]["mark_cross"] >= 1


def test_segment_placements(O):
    seen = []
    for k, scan in enumerate(SEG_SCANS):
        for j, (n, e) in enumerate(SEG_SPECS[6 * k:6 * k + 6]):
            ends = FL.segment_ends(scan.livox, j)
            assert scan.line_lengths[j] == n
            if e is None:
                assert ends[:2] == [99, 119] and 99 // 64 == 119 // 64      # two boundaries inside the round 64 .. 127
            elif e >= 0:
                assert ends[0] == e, (k, j, ends)
                seen.append((n, e))
    assert sorted(set(e for n, e in seen if n == 600)) == [63, 64, 65, 255, 256, 257, 261, 594]
    assert sorted(set(e for n, e in seen if n == 3300)) == [63, 64, 65, 255, 256, 257, 261, 3294]
    # the other raw orders cut long lines too: a "seq" line of 6 500 points lies in two or three blocks
    long_seq = [len(FL.segment_ends(s.livox, j)) for s in FORM_SCANS if s.order == "seq" for j, n in enumerate(s.line_lengths) if n >= 4097]
    assert long_seq and min(long_seq) >= 1


SHORT = [n for n in FL.ALL_LENGTHS if n <= 700]


@pytest.mark.parametrize("n", SHORT)
def test_oracle_equals_the_second_restatement_on_the_short_lines(O, n):
    for scan in FORM_SCANS:
        for kind, lid, m in scan.lengths():
            if m != n:
                continue
            pts = (scan.rings if kind == "ring" else scan.lines)[lid]
            so, fo, flo = O.detect_feature_points(pts)
            sp, fp, flp = second_opinion.detect_feature_points_py(pts)
            assert np.array_equal(flo, np.asarray(flp, np.int32).reshape(-1)[:n]), (scan.name, kind, lid)
            assert list(so) == list(sp) and list(fo) == list(fp), (scan.name, kind, lid)
