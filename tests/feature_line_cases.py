"""Scan lines of exactly chosen length for the feature front end (csrc/feature.hip: bucketing, k_stencil, k_select_part, k_select), the
scans that carry them, and a plain restatement of which kernel form a line of n points takes.  numpy only at module level: no oracle,
no project header (the functions that need the oracle or the synth module take them as arguments).

  line_points(rng, n, style)      one scan line of exactly n points, (n, 4) float32, with every branch of the selection live: flat
                                  stretches whose point spacing lets marks propagate, corners (150), range jumps over 1 m (100 / 101),
                                  grazing stretches, points beyond 50 m and nearer than 1 m, repeated points, quantised reflectivity.
                                  style "boundary" lays a flat run across every partition boundary 5 + (n - 11) j / 50 and puts a corner or
                                  a break within 3 points of two boundaries in three; style "crop" puts stretches on both sides of 2 m and 50 m.
  velo_rings / velo_scan_of       rings at the exact pitch of their ring id, raw scan in column-interleaved order
  livox_scan_of(lines, order)     LIVOX_DTYPE records, line id j holds exactly lines[j]; order "rr", "seq" or an explicit placement of a
                                  line's records into the 4096-record raw blocks (one segment of the line per block: segment_ends)
  expected_form(...)              part64 | part128 | listed-lds | listed-scratch | direct-lds | direct-scratch (| none for an empty line)
  TABLES, *_scans()               the lengths at which a rule of the dispatch decides, and the scans the GPU tests walk

The contexts of the tests are created with NEAR / FAR as thresholds (nothing is cropped, the `depth > 50` branches of the selection still
run on the points beyond 50 m), so the fused cloud's per-ring counts are the line lengths."""
import zlib

import numpy as np

F32 = np.float32
NEAR, FAR = 0.05, 1000.0          # near_th / far_th of the contexts and of the oracle calls: every point of every line is kept
N_RINGS, N_LINES = 16, 6          # the default layout
PITCH0, PITCH_STEP = -15.0, 2.0
MAX_VELO, MAX_LIVOX = 16 * 1800, 24000   # mml_config_default (csrc/capi.hip:82-83)
RAW_BLOCK = 4096                  # MML_OP_BLK: the one-pass bucketing stores one segment of a line per raw block of this many points
LIVOX_DTYPE = np.dtype([("offset_time", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                        ("reflectivity", "u1"), ("tag", "u1"), ("line", "u1"), ("_pad", "u1")])

# ---- the dispatch, restated (constants as literals; the line of csrc/feature.hip each comes from) ----------------------------------
PARTS = 50                        # :3316  partition j spans 5 + range * j / 50 .. 5 + range * (j + 1) / 50 - 1, range = n - 11 (:3231)
SEGMENT_MAX_SLOTS = 16            # :1855  ST_SEGMENT_MAX_SLOTS: calls of up to 16 slots take stencil modes 1 + 2 and the direct k_select
ST_TILE = 256                     # :1850  positions per stencil tile (5-point halo on each side)
PART64 = (161, 3211)              # :3232  150 <= n - 11 <= 50 * 64
PART128 = (3212, 6411)            # :3232  .. <= 50 * 128, what the narrow form left (:3237)
SP_LINES, SP_LINES_WIDE = 4, 2    # :3623  lines per workgroup of the narrow / the wide form
SEL_ROWS = (256, 128)             # :3125-3126  workgroups of the list-mode k_select: rings, Livox lines
SEL_CAP, SEL_CAP_VELO = 4096, 2048   # :4205-4212 for the default layout: 51 * (24000 / 6) / 50 -> 4096; 1800 * 9 / 8 -> 2048
NOMINAL = 2 * ((MAX_VELO + MAX_LIVOX) // (N_RINGS + N_LINES)) + ST_TILE   # :4025  segment-mode stencil grid, in positions: 5056


def sel_caps(max_velo_points=MAX_VELO, max_livox_points=MAX_LIVOX, n_rings=N_RINGS, n_lines=N_LINES):
    """(sel_cap, sel_cap_velo) as mml_feature_init (:4205-4212) sets them: whole multiples of 512 points per workgroup"""
    def round_cap(want):                                    # :3639 select_round_cap
        for k in (2, 4, 6, 8, 12, 16, 24):
            if k * 512 >= want:
                return k * 512
        return 24 * 512
    nv, nl = (max_velo_points + 63) & ~63, (max_livox_points + 63) & ~63
    ring_nominal = nv // n_rings
    cap = round_cap(max(51 * (nl // n_lines) // 50, 2 * ring_nominal))
    return cap, min(round_cap(ring_nominal * 9 // 8), cap)


def expected_form(n, count, kind, sel_cap=SEL_CAP, sel_cap_velo=SEL_CAP_VELO):
    """The selection form a line of n points takes in a call of `count` slots; kind "ring" or "livox".
    count > 16 (:4057): k_select_part narrow, then wide, then k_select_list + list-mode k_select, which runs the sel_cap_velo variant on
    the listed rings and the sel_cap variant on the listed Livox lines (:4072-4074); LDS for n <= cap, global scratch beyond (:3154).
    count <= 16 (:4075): ONE launch of the sel_cap variant over rings and Livox lines.  (The branch behind it, rings on the sel_cap_velo
    variant, needs a layout without Livox lines or sel_cap < sel_cap_velo: mml_create refuses the first, :4212 rules out the second.)"""
    assert kind in ("ring", "livox")
    if n <= 0:
        return "none"                                       # :1880, :3148, :3173: nothing runs on an empty line
    if count > SEGMENT_MAX_SLOTS:
        if PART64[0] <= n <= PART64[1]:
            return "part64"
        if PART128[0] <= n <= PART128[1]:
            return "part128"
        return "listed-lds" if n <= (sel_cap_velo if kind == "ring" else sel_cap) else "listed-scratch"
    return "direct-lds" if n <= sel_cap else "direct-scratch"


def partition_starts(n):
    """the 51 boundaries 5 + (n - 11) * j / 50 (C integer division of a non-negative product), j = 0 .. 50"""
    assert n >= 11
    return np.array([5 + (n - 11) * j // PARTS for j in range(PARTS + 1)])


def partition_sizes(n):
    return np.diff(partition_starts(n))


# ---- the length tables: the smallest shapes at which each rule can go wrong -------------------------------------------------------------
TABLES = {
    "interior": [0, 1, 10, 11, 12, 16],                                  # nothing / the stencil's interior 5 <= i < n - 5
    "part64_lower": [160, 161, 162],
    "windows": [191, 192, 193, 511, 512, 513, 575, 576, 577],            # nwin = (n + 63) >> 6, eight windows per turn
    "tiles": [ST_TILE * m + d for m in (1, 2) for d in (-6, -5, -1, 0, 1, 5, 6, 10, 11)],
    "part64_part128": [3210, 3211, 3212, 3213],
    "windows_wide": [3199, 3200, 3201, 3263, 3264, 3265],
    "part128_upper": [6410, 6411, 6412, 6413],
    "direct_caps": [SEL_CAP_VELO - 1, SEL_CAP_VELO, SEL_CAP_VELO + 1, SEL_CAP - 1, SEL_CAP, SEL_CAP + 1],
    "segment_grid": [NOMINAL - 1, NOMINAL, NOMINAL + 1, NOMINAL + 257],
    "largest": [6500],
}
ALL_LENGTHS = sorted({n for t in TABLES.values() for n in t}, reverse=True)
# partition sizes the tables claim: n - 11 = 150: all 3; 3200: all 64; 3201: one 65; 6400: all 128; 6401: one 129
PARTITION_CLAIMS = {161: (3, 3, 0), 3211: (64, 64, 0), 3212: (64, 65, 1), 6411: (128, 128, 0), 6412: (128, 129, 1)}   # n: (min, max, how many at max if > min)


# ---- lines ---------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def sweep_az(n):
    """azimuths of a Livox-like line: a triangle wave inside +-1.1 rad (x stays positive: the reference drops records with x < 0.01) at
    0.0015 rad per point -- 2 cm at 12 m, so marks propagate, and 4 points span more than the 5 cm the corner test asks for"""
    t = np.arange(n) * 0.0015 + 0.4
    return 1.1 - np.abs((t % 4.4) - 2.2)


def ring_az(n, ncols):
    """azimuths of the first n columns of a Velodyne-like sweep of max(ncols, 1800) columns, clockwise"""
    return -(2.0 * np.pi / max(ncols, 1800)) * np.arange(n) - 0.01


def _plane(az, a0, r0, theta):
    """range of a wall that the ray at azimuth a0 meets at r0 under incidence theta"""
    return r0 * np.cos(theta) / np.maximum(np.cos(az - a0 + theta), 0.05)


def _mixed_ranges(rng, az, bases):
    n = len(az)
    r = np.empty(n)
    i = 0
    while i < n:
        seg = int(rng.integers(5, 90))
        kind = int(rng.integers(0, 8))
        a = az[i:i + seg]
        base = float(rng.choice(bases)) if bases is not None else float(rng.uniform(2.5, 12.0))
        if kind == 0:      # wall at an angle
            v = _plane(a, a[0], base, rng.uniform(-1.0, 1.0))
        elif kind == 1:    # constant range
            v = np.full(len(a), base)
        elif kind == 2:    # corner: two planes meeting inside the segment
            h = len(a) // 2
            v = np.where(np.arange(len(a)) < h, _plane(a, a[h], base, 0.8 * np.sign(a[-1] - a[0] + 1e-12)),
                         _plane(a, a[h], base, -0.8 * np.sign(a[-1] - a[0] + 1e-12)))
        elif kind == 3:    # noisy vegetation
            v = base + rng.normal(0, 0.3, len(a))
        elif kind == 4:    # slow ramp
            v = base + np.linspace(0, rng.uniform(-1, 1), len(a))
        elif kind == 5:    # beyond 50 m
            v = _plane(a, a[0], rng.uniform(51.0, 70.0), rng.uniform(-0.3, 0.3))
        elif kind == 6:    # grazing incidence
            v = _plane(a, a[0], base, rng.choice([-1.0, 1.0]) * rng.uniform(1.35, 1.5))
        else:              # nearer than 1 m
            v = np.full(len(a), rng.uniform(0.4, 0.95))
        r[i:i + seg] = v + rng.normal(0, rng.choice([0.0, 0.002, 0.01]), len(a))
        i += seg
    return r


def _boundary_ranges(rng, az, n):
    """long flat walls; a flat run across every partition boundary; a break or a corner within 3 points of two boundaries in three"""
    r = np.empty(n)
    i = 0
    while i < n:
        seg = int(rng.integers(100, 400))
        a = az[i:i + seg]
        r[i:i + seg] = _plane(a, a[len(a) // 2], rng.uniform(7.0, 12.0), rng.uniform(-0.5, 0.5))
        i += seg
    r += rng.normal(0, 0.001, n)
    if n < 23:
        return r
    for j, b in enumerate(partition_starts(n)):
        k = int(b) + int(rng.integers(-3, 4))
        if j % 3 == 1 and 6 <= k < n - 12:           # a pillar in front of the wall: range jumps of 2 m at k and behind it
            r[k:k + int(rng.integers(5, 11))] -= 2.0
        elif j % 3 == 2 and 9 <= k < n - 9:          # two planes meeting at k
            w = slice(k - 8, k + 9)
            s = 0.8 * np.sign(az[k + 1] - az[k - 1] + 1e-12)
            r[w] = np.where(np.arange(k - 8, k + 9) < k, _plane(az[w], az[k], r[k], s), _plane(az[w], az[k], r[k], -s))
    return r


def line_points(rng, n, style="mixed", az=None, pitch_deg=None):
    """One scan line of exactly n points: (n, 4) float32 x, y, z, intensity (whole numbers 0 .. 255: Livox reflectivity is a byte).
    az: the azimuth of every point (sweep_az(n) when not given); pitch_deg: the points lie on the cone of that pitch (a ring)."""
    assert style in ("mixed", "boundary", "crop")
    if n == 0:
        return np.zeros((0, 4), F32)
    az = sweep_az(n) if az is None else np.asarray(az, np.float64)
    assert len(az) == n
    if style == "boundary":
        rho = _boundary_ranges(rng, az, n)
    else:
        rho = _mixed_ranges(rng, az, [1.6, 1.9, 1.99, 2.01, 2.1, 3.0, 8.0, 49.0, 49.9, 50.1, 51.0] if style == "crop" else None)
    rho = np.clip(rho, 0.3, 120.0)
    z = rho * np.tan(np.deg2rad(pitch_deg)) if pitch_deg is not None else -0.4 + 0.03 * np.sin(5.0 * az)
    inten = [np.zeros(n), np.round(rng.uniform(0, 255, n)), np.round(rng.uniform(0, 3, n)) * 80.0][int(rng.integers(0, 3))]
    pts = np.stack([rho * np.cos(az), rho * np.sin(az), z, inten], 1).astype(F32)
    for _ in range(int(rng.integers(0, 4)) if n > 12 else 0):   # repeated points (zero-length neighbour vectors)
        j = int(rng.integers(0, n - 6))
        pts[j:j + int(rng.integers(2, 6))] = pts[j]
    return pts


def velo_rings(rng, lengths, style="mixed"):
    """ring r of len(lengths) rings: lengths[r] points at the ring's pitch, in the first lengths[r] columns of one common sweep"""
    ncols = max(list(lengths) + [0])
    return [line_points(rng, n, style, az=ring_az(n, ncols), pitch_deg=PITCH0 + PITCH_STEP * r) for r, n in enumerate(lengths)]


def velo_scan_of(rings, pitch0=PITCH0, pitch_step=PITCH_STEP):
    """(sum of lengths, 4) float32 raw scan in column-interleaved order: column c holds the rings with more than c points, ring id ascending.
    Every point must sit at its ring's pitch to well inside the +-half-step the ring id is rounded with."""
    col, rid, rows = [], [], []
    for r, pts in enumerate(rings):
        pts = np.ascontiguousarray(pts, F32).reshape(-1, 4)
        if len(pts):
            ang = np.rad2deg(np.arctan2(pts[:, 2].astype(np.float64), np.hypot(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64))))
            assert np.abs(ang - (pitch0 + pitch_step * r)).max() < 0.01 * pitch_step, r
        col.append(np.arange(len(pts)))
        rid.append(np.full(len(pts), r))
        rows.append(pts)
    col, rid, rows = np.concatenate(col), np.concatenate(rid), np.concatenate(rows)
    return np.ascontiguousarray(rows[np.lexsort((rid, col))])


FILLER_LINE = 7      # a line id beyond the layout's: the reference (and the device) skip the record


def livox_scan_of(lines, order="rr"):
    """LIVOX_DTYPE records in which line id j holds exactly lines[j] (in order).  order:
      "rr"     round-robin over the lines that still have points          "seq"    line after line
      dict     explicit placement {line id: [c0, c1, ...]}: c_b records of the line go into raw block b (4096 records each), the rest of the
               line into the blocks behind its last explicit one wherever there is room; lines not named are placed like a rest from block
               0 on.  Blocks are filled up with records of line id 7, which every consumer skips.
    offset_time is linear in the raw index (whole nanoseconds, 0.1 s over 24 000 records)."""
    lines = [np.ascontiguousarray(l, F32).reshape(-1, 4) for l in lines]
    lens = [len(l) for l in lines]
    if order == "rr":
        idx = np.concatenate([np.arange(n) for n in lens] + [np.zeros(0, np.int64)])
        lid = np.concatenate([np.full(n, j) for j, n in enumerate(lens)] + [np.zeros(0, np.int64)])
        o = np.lexsort((lid, idx))
        lid, idx = lid[o], idx[o]
    elif order == "seq":
        idx = np.concatenate([np.arange(n) for n in lens] + [np.zeros(0, np.int64)])
        lid = np.concatenate([np.full(n, j) for j, n in enumerate(lens)] + [np.zeros(0, np.int64)])
    else:
        heads = {j: list(order.get(j, [])) for j in range(len(lines))}
        assert all(sum(h) <= lens[j] for j, h in heads.items())
        placed = [0] * len(lines)
        lid, idx = [], []
        b = 0
        while any(placed[j] < lens[j] for j in range(len(lines))):
            room = RAW_BLOCK
            for j in range(len(lines)):                       # the explicit counts of this block
                c = heads[j][b] if b < len(heads[j]) else 0
                lid += [j] * c
                idx += range(placed[j], placed[j] + c)
                placed[j] += c
                room -= c
            assert room >= 0, "block %d overfull" % b
            for j in range(len(lines)):                       # rests of the lines whose explicit blocks lie in front
                if b >= len(heads[j]) and placed[j] < lens[j] and room > 0:
                    c = min(room, lens[j] - placed[j])
                    lid += [j] * c
                    idx += range(placed[j], placed[j] + c)
                    placed[j] += c
                    room -= c
            if any(placed[j] < lens[j] for j in range(len(lines))):
                lid += [FILLER_LINE] * room                   # not the last block: fill it up
                idx += [0] * room
            b += 1
        lid, idx = np.array(lid, np.int64), np.array(idx, np.int64)
    out = np.zeros(len(lid), LIVOX_DTYPE)
    assert len(out) <= MAX_LIVOX, len(out)
    out["offset_time"] = np.round(np.arange(len(out)) * (1e8 / 24000.0)).astype(np.uint32) + 1000
    out["line"] = lid
    out["x"], out["y"], out["z"] = 1.0, 0.0, 0.0
    for j, l in enumerate(lines):
        m = lid == j
        if len(l):
            assert l[:, 0].min() >= 0.01 and np.array_equal(l[:, 3], np.round(l[:, 3])) and 0 <= l[:, 3].min() and l[:, 3].max() <= 255
        out["x"][m], out["y"][m], out["z"][m] = l[idx[m], 0], l[idx[m], 1], l[idx[m], 2]
        out["reflectivity"][m] = l[idx[m], 3].astype(np.uint8)
    return out


def segment_ends(livox, line):
    """last line index of every segment of the line but the last: where consecutive points of the line lie in different raw blocks"""
    blk = np.flatnonzero(livox["line"] == line) // RAW_BLOCK
    return [int(i) for i in np.flatnonzero(np.diff(blk))]


# ---- scans ---------------------------------------------------------------------------------------------------------------------------
class Scan:
    """16 rings + 6 Livox lines of given lengths (None: the sensor is absent).  crop: built for the default thresholds (2 m, 50 m)."""

    def __init__(self, name, ring_lengths, line_lengths, style="mixed", order="rr", crop=False):
        assert ring_lengths is None or (len(ring_lengths) == N_RINGS and sum(ring_lengths) <= MAX_VELO), (name, sum(ring_lengths or []))
        assert line_lengths is None or len(line_lengths) == N_LINES, name
        self.name, self.ring_lengths, self.line_lengths, self.style, self.order, self.crop = name, ring_lengths, line_lengths, style, order, crop
        self._built = None

    def _build(self):
        if self._built is None:
            rng = _rng("scan", self.name)
            rings = velo_rings(rng, self.ring_lengths, self.style) if self.ring_lengths is not None else None
            lines = [line_points(rng, n, self.style) for n in self.line_lengths] if self.line_lengths is not None else None
            velo = velo_scan_of(rings) if rings is not None else None
            livox = livox_scan_of(lines, self.order) if lines is not None else None
            if velo is not None and len(velo) == 0:
                velo = None
            if livox is not None and len(livox) == 0:
                livox = None
            self._built = (rings, lines, velo, livox)
        return self._built

    rings = property(lambda self: self._build()[0])
    lines = property(lambda self: self._build()[1])
    velo = property(lambda self: self._build()[2])
    livox = property(lambda self: self._build()[3])

    @property
    def thresholds(self):
        return (2.0, 50.0) if self.crop else (NEAR, FAR)

    def lengths(self):
        """[(kind, line id, n)] of the scan's lines"""
        return [("ring", r, n) for r, n in enumerate(self.ring_lengths or [])] + [("livox", j, n) for j, n in enumerate(self.line_lengths or [])]


_ORACLE = {}   # one oracle record per scan, shared by every test that needs it


def oracle_fused(O, scan):
    """What extract + undistort (identity) + downsample must leave behind for the scan: the oracle's fused cloud (rings, then lines), the
    four label counts, the cloud after the identity undistortion and both down-sampled stacks."""
    if scan.name not in _ORACLE:
        near, far = scan.thresholds
        ev = O.extract_velo(scan.velo, near=near, far=far) if scan.velo is not None else None
        el = O.extract_livox(scan.livox, near=near, far=far) if scan.livox is not None else None
        parts = [e for e in (ev, el) if e is not None]
        o = {k: np.concatenate([e[k] for e in parts]) for k in ("xyzi", "label", "reltime", "ring")}
        o["counts"] = ((ev["n_corner"], ev["n_surf"]) if ev else (0, 0)) + ((el["n_corner"], el["n_surf"]) if el else (0, 0))
        o["n_velo"] = len(ev["xyzi"]) if ev else 0
        o["und"] = O.undistort(o["xyzi"][:, :3], o["reltime"], np.eye(3), np.zeros(3))
        o["corner"] = O.voxel_downsample(o["und"][o["label"] == 1], 0.4)
        o["surf"] = O.voxel_downsample(o["und"][o["label"] == 2], 0.2)
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ORACLE[scan.name] = o
    return _ORACLE[scan.name]


RING_FILL = [1750, 1400, 1100, 820, 640, 333, 170, 150, 90, 37, 5, 700]


def form_scans():
    """12 scans that together hold every length of the tables once as a ring and once as a Livox line: scan k takes every 12th length
    (longest first) for its rings and the same stride six places on for its lines, so that a scan mixes the forms; the other rings hold
    ordinary lengths.  Ring ids and line ids rotate with k; styles and raw orders alternate."""
    out = []
    for k in range(12):
        ring_t, line_t = ALL_LENGTHS[k::12], ALL_LENGTHS[(k + 6) % 12::12]
        rings = [None] * N_RINGS
        for i, n in enumerate(ring_t):
            rings[(k + 3 * i) % N_RINGS] = n
        fill = iter(RING_FILL[k % 3:] + RING_FILL)
        rings = [n if n is not None else next(fill) for n in rings]
        lines = [None] * N_LINES
        for i, n in enumerate(line_t):
            lines[(k + i) % N_LINES] = n
        lines = [n if n is not None else 700 + 13 * k for n in lines]
        out.append(Scan("forms%d" % k, rings, lines, style=("mixed", "boundary")[k % 2], order=("seq", "rr", "rr")[k % 3]))
    return out


def crop_scans():
    """the pair for a context with the DEFAULT thresholds: points on both sides of 2 m and 50 m on lines at the length edges"""
    a = Scan("crop0", [3212, 161, 2048, 512, 160, 3211, 256, 11, 2049, 577, 1000, 700, 261, 12, 900, 3200],
             [3211, 6411, 160, 4097, 512, 3212], style="crop", order="rr", crop=True)
    b = Scan("crop1", [6412, 162, 3213, 192, 10, 250, 4096, 1800, 513, 3201, 0, 16, 1500, 2047, 266, 400],
             [6412, 161, 3200, 4096, 267, 1], style="crop", order="seq", crop=True)
    return [a, b]


def listed_scans():
    """four scans whose 16 rings and 6 lines are all listed for k_select in a batch: 1 .. 160 points, or 6412 and more where the slot holds
    them (four rings / three lines)"""
    rng = _rng("listed")
    out = []
    for k in range(4):
        rings = [int(v) for v in rng.integers(1, 161, N_RINGS)]
        lines = [int(v) for v in rng.integers(1, 161, N_LINES)]
        rings[k], rings[15 - k] = 160, 12
        lines[k] = 160
        if k == 1:
            for r, n in zip((0, 5, 10, 15), (6412, 6413, 6500, 6412)):
                rings[r] = n
        if k == 2:
            for j, n in zip((1, 3, 4), (6412, 6413, 7000)):
                lines[j] = n
        out.append(Scan("listed%d" % k, rings, lines, style=("mixed", "boundary")[k % 2], order=("rr", "seq")[k % 2]))
    return out


def eligible_scans():
    """three scans with every line inside 161 .. 6411: nothing is listed"""
    out = []
    for k in range(3):
        rings = [161 + 97 * ((5 * r + k) % 16) for r in range(N_RINGS)]
        rings[k], rings[8 + k] = 3211 + k, 3212 - k
        lines = [161 + k, 3211, 3212, 6411 - 900 * k, 2000 + k, 3300]
        out.append(Scan("eligible%d" % k, rings, lines[k:] + lines[:k], style=("boundary", "mixed")[k % 2], order=("rr", "seq")[k % 2]))
    return out


def handover_scans():
    """narrow / wide / listed alternating over consecutive line ids 0 .. 21 (rings 0 .. 15, Livox lines as ids 16 .. 21: ids 20 and 21 are
    the ragged last group of the narrow form's four lines per workgroup), in the three rotations of the pattern"""
    narrow = [161, 700, 162, 900, 512, 163, 3211, 3200]    # (the first six places go to rings: 16 rings hold five or six wide ones only
    wide = [3212, 3213, 3212, 3214, 3213, 3212, 6411, 3264]  #  next to short narrow ones and one listed ring of 6412 points)
    listed = [160, 6412, 12, 100, 1, 37, 6413, 159]
    out = []
    for rot in range(3):
        pick = [(narrow, wide, listed)[(i + rot) % 3][i // 3] for i in range(N_RINGS + N_LINES)]
        rings, lines = pick[:N_RINGS], pick[N_RINGS:]
        out.append(Scan("handover%d" % rot, rings, lines, style=("boundary", "mixed", "boundary")[rot], order=("rr", "seq", "rr")[rot]))
    return out


SEGMENT_ENDS = [63, 64, 65, 255, 256, 257, 261]   # last line index of a line's first segment (261: the halo of the stencil's second tile)


def segment_scans():
    """Livox lines of 600 and 3300 points whose first segment ends at a chosen line index (SEGMENT_ENDS and n - 6), and one line of three
    segments with two boundaries inside one 64-index round (after indices 99 and 119): the general translation path at a chosen place"""
    ends = SEGMENT_ENDS + [None]
    specs = [(n, (n - 6 if e is None else e)) for e in ends for n in (600, 3300)]       # 16 (length, end of the first segment)
    specs += [(600, None), (777, -1)]                                                   # three segments; an ordinary line
    out = []
    for k in range(3):
        mine = specs[6 * k:6 * k + 6]
        order = {}
        for j, (n, e) in enumerate(mine):
            if e is None:
                order[j] = [100, 20]
            elif e >= 0:
                order[j] = [e + 1] if e < 2000 else [0, e + 1]   # (a first segment too long to share block 0 lies in block 1)
        rings = [161 + 61 * ((3 * r + k) % 16) for r in range(N_RINGS)]
        out.append(Scan("segments%d" % k, rings, [n for n, _ in mine], style=("mixed", "boundary", "mixed")[k], order=order))
    return out, specs
