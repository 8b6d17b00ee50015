"""Inputs and the numpy restatement shared by tests/test_wire_batch_host.py and tests/test_gpu_wire_batch.py: union_cloud messages
in wire form (PointCloud2 payloads of any point_step, 19- / 20-byte Livox records), laid out in one buffer per sensor with frame
starts at every residue mod 4 and 0xA5-filled gaps between the payloads.  Everything is compared as uint32 words / bytes."""
import numpy as np

# float32 bit patterns that only survive a decode made of moves: quiet and signalling NaNs with payloads (both signs), +-0,
# denormals (smallest, largest, negative), +-inf, the largest finite value, 1.0
SPECIAL = np.array([0x7fc12345, 0x7f812345, 0xffc00001, 0xff800001, 0x7fffffff, 0x7f800001, 0x00000000, 0x80000000, 0x00000001,
                    0x007fffff, 0x807fffff, 0x7f800000, 0xff800000, 0x7f7fffff, 0x3f800000], np.uint32)


def velo_payload(rng, n, step, offs):
    """n records of `step` random bytes; the first records carry SPECIAL in every field, rotated from field to field."""
    rec = rng.integers(0, 256, (n, step), dtype=np.uint8)
    k = min(n, len(SPECIAL))
    for j, o in enumerate(offs):
        if o >= 0 and k:
            rec[:k, o:o + 4] = np.roll(SPECIAL, j)[:k].astype("<u4").view(np.uint8).reshape(k, 4)
    return rec.reshape(-1)


def livox_payload(rng, n, rec_bytes):
    """n records of 19 or 20 random bytes: SPECIAL in x, y, z of the first records; with n >= 256 every value 0 .. 255 occurs in
    reflectivity, tag and line (at different rows for each)."""
    rec = rng.integers(0, 256, (n, rec_bytes), dtype=np.uint8)
    k = min(n, len(SPECIAL))
    for j in range(3):
        if k:
            rec[:k, 4 + 4 * j:8 + 4 * j] = np.roll(SPECIAL, j)[:k].astype("<u4").view(np.uint8).reshape(k, 4)
    if n >= 256:
        i = np.arange(n)
        rec[:, 16], rec[:, 17], rec[:, 18] = i & 255, (i + 85) & 255, (255 - i) & 255
    return rec.reshape(-1)


def lay_out(payloads, first_residue=0, gaps=True, lead=True):
    """One buffer holding the payloads in order: frame i starts at residue (first_residue + i) mod 4, behind a gap of 0xA5 bytes
    (4 .. 7 bytes with `gaps`, else only what the residue needs); `lead`: a gap in front of the first payload too.  The buffer
    ends on the last payload's last byte.  Returns (uint8 buffer, int64 offsets); an empty frame gets the running position."""
    out, at, pos = [], [], 0
    for i, p in enumerate(payloads):
        want = (first_residue + i) & 3
        pad = (want - pos) & 3
        if gaps and (i > 0 or lead):
            pad += 4
        if i == 0 and not lead:
            pad = 0
        if len(p) == 0:
            pad = 0
        out.append(np.full(pad, 0xA5, np.uint8))
        pos += pad
        at.append(pos)
        out.append(np.asarray(p, np.uint8))
        pos += len(p)
    buf = np.concatenate(out) if out else np.zeros(0, np.uint8)
    return np.ascontiguousarray(buf), np.array(at, np.int64)


def ref_velo(data, at, n, step, offs):
    """The numpy restatement of the Velodyne decode: (sum n, 4) uint32 words x, y, z, intensity, frame after frame."""
    rows = []
    for a, k in zip(at, n):
        rec = np.frombuffer(bytes(data[a:a + k * step]), np.uint8).reshape(k, step)
        cols = [np.ascontiguousarray(rec[:, o:o + 4]).view("<u4").reshape(k) if o >= 0 else np.zeros(k, np.uint32) for o in offs]
        rows.append(np.stack(cols, 1).astype(np.uint32).reshape(k, 4))
    return np.concatenate(rows) if rows else np.zeros((0, 4), np.uint32)


def ref_livox(data, at, n, rec_bytes):
    """The same for the Livox decode: (sum n, 5) uint32 words of the 20-byte struct; the 19-byte form gets a zero pad byte."""
    rows = []
    for a, k in zip(at, n):
        rec = np.frombuffer(bytes(data[a:a + k * rec_bytes]), np.uint8).reshape(k, rec_bytes)
        full = np.zeros((k, 20), np.uint8)
        full[:, :rec_bytes] = rec
        rows.append(full.view("<u4").reshape(k, 5))
    return np.concatenate(rows) if rows else np.zeros((0, 5), np.uint32)


def words(a):
    """Any array of 4-byte-multiple records as rows of uint32."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1).view("<u4")


def make_call(rng, n_velo, n_livox, step, offs, rec_bytes, first_residue=0, gaps=True, lead=True):
    """A whole call: random payloads of the given counts, laid out.  Returns a dict with the arguments of the three entry points
    (velo_data, velo_at, n_velo, point_step, offs, livox_data, livox_at, n_livox, livox_record_bytes) under `args`, plus the
    per-frame reference words `velo` / `livox` (lists)."""
    vp = [velo_payload(rng, k, step, offs) for k in n_velo]
    lp = [livox_payload(rng, k, rec_bytes) for k in n_livox]
    vd, va = lay_out(vp, first_residue, gaps, lead)
    ld, la = lay_out(lp, first_residue + 1, gaps, lead)
    nv, nl = np.array(n_velo, np.int32), np.array(n_livox, np.int32)
    return dict(args=(vd if len(vd) else None, va, nv, step, tuple(offs), ld if len(ld) else None, la, nl, rec_bytes),
                velo=[ref_velo(vd, [a], [k], step, offs) for a, k in zip(va, nv)],
                livox=[ref_livox(ld, [a], [k], rec_bytes) for a, k in zip(la, nl)])
