"""mml_scan_upload_wire_batch on the device: `count` union_cloud messages in wire form into `count` slots in one call, held equal --
byte for byte -- to the single calls (mml_scan_upload_wire, mml_scan_upload_pointcloud2) on a second context and to the host
decode.  Small contexts (8 slots x 512 + 512 points); the out-of-range cases are all refused on the host before any launch."""
import numpy as np
import pytest

import wire_cases as W

pytestmark = pytest.mark.gpu

CAP = 512
BASE_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 512]
# (point_step, field offsets, livox_record_bytes): 19 is held against mml_scan_upload_wire, 20 against mml_scan_upload_pointcloud2
CASES = [(12, (8, 0, 4, -1), 19), (19, (1, 6, 11, 15), 20), (22, (0, 4, 8, 12), 19), (32, (5, 26, 11, 18), 20), (256, (252, 129, 2, 67), 19),
         (22, (18, 2, 13, 7), 20)]


# Points per frame, per case: every count of BASE_COUNTS for both sensors, which holds the kernel's tile size (256 records whatever
# the record size) with its neighbours 255 and 257; 512 is two whole tiles.
# Frame 2 has an empty Velodyne part, frame 4 an empty Livox part, frame 6 is empty.
N_VELO = [[1, 64, 0, 257, 63, 512, 0, 255], [65, 256, 0, 512, 1, 63, 0, 257], [255, 65, 0, 64, 512, 256, 0, 1],
          [511, 512, 0, 257, 255, 65, 0, 63], [63, 64, 0, 65, 512, 257, 0, 256], [512, 1, 0, 255, 64, 63, 0, 65]]
N_LIVOX = [[512, 255, 65, 1, 0, 64, 0, 257], [63, 512, 256, 65, 0, 1, 0, 255], [0, 257, 64, 512, 0, 63, 0, 256],
           [257, 1, 512, 0, 0, 256, 0, 64], [256, 64, 63, 255, 0, 512, 0, 65], [1, 65, 257, 63, 0, 255, 0, 512]]


def _counts(M, case_index, step, rec):
    return list(N_VELO[case_index]), list(N_LIVOX[case_index])


def test_every_count_is_tried(M):
    seen_v, seen_l = set(), set()
    for i, (step, _, rec) in enumerate(CASES):
        nv, nl = _counts(M, i, step, rec)
        seen_v |= set(nv)
        seen_l |= set(nl)
        assert nv[2] == 0 and nl[2] > 0 and nl[4] == 0 and nv[4] > 0 and nv[6] == nl[6] == 0 and max(nv + nl) <= CAP
    t = M.WIRE_TILE_POINTS
    assert seen_v >= set(BASE_COUNTS) >= {t - 1, t, t + 1, 2 * t} and seen_l >= set(BASE_COUNTS)


def _ctx(M, **over):
    return M.Context(max_scans=8, max_velo_points=CAP, max_livox_points=CAP, **over)


def _single(M, ctx, slot, args, i):
    """Frame i of a call through the single-message entry points."""
    vd, va, nv, step, offs, ld, la, nl, rec = args
    v = vd[va[i]:va[i] + nv[i] * step].copy() if nv[i] else np.zeros(0, np.uint8)
    l = ld[la[i]:la[i] + nl[i] * rec].copy() if nl[i] else np.zeros(0, np.uint8)
    if rec == 19:
        ctx.scan_upload_wire(slot, v, int(nv[i]), step, *offs, l, int(nl[i]))
    else:
        ctx.scan_upload_pointcloud2(slot, v, int(nv[i]), step, *offs, np.frombuffer(l.tobytes(), M.LIVOX_DTYPE) if nl[i] else None)


def _raw_words(ctx, slot):
    v, l = ctx.scan_raw_download(slot)
    return (W.words(v) if len(v) else np.zeros((0, 4), np.uint32)), (W.words(l) if len(l) else np.zeros((0, 5), np.uint32))


@pytest.mark.parametrize("case_index", range(len(CASES)))
def test_batch_equals_single_calls_and_host(M, case_index):
    step, offs, rec = CASES[case_index]
    nv, nl = _counts(M, case_index, step, rec)
    call = W.make_call(np.random.default_rng(40 + case_index), nv, nl, step, offs, rec, first_residue=case_index)
    hv, hl = M.wire_decode_host(*call["args"])
    ev, el = np.cumsum([0] + nv), np.cumsum([0] + nl)
    a, b = _ctx(M), _ctx(M)
    try:
        a.scan_upload_wire_batch(0, *call["args"])
        for i in range(8):
            _single(M, b, i, call["args"], i)
        for i in range(8):
            av, al = _raw_words(a, i)
            bv, bl = _raw_words(b, i)
            assert av.shape == (nv[i], 4) and al.shape == (nl[i], 5)
            assert np.array_equal(av, bv) and np.array_equal(al, bl), i
            assert np.array_equal(av, call["velo"][i]) and np.array_equal(al, call["livox"][i]), i
            assert np.array_equal(av, W.words(hv[ev[i]:ev[i + 1]]) if nv[i] else av) and np.array_equal(al, W.words(hl[el[i]:el[i + 1]]) if nl[i] else al)
    finally:
        a.close()
        b.close()


def _known(synth, k):
    return synth.velo_scan(k, n_az=32), synth.livox_scan(k, n=CAP)   # 16 rings x 32 azimuths = 512 points, 512 Livox points


def _as_wire(frames, step=22):
    """Scans (velo n x 4 float32, livox LIVOX_DTYPE) as a wire-form call with 19-byte Livox records."""
    vp, lp = [], []
    for v, l in frames:
        rec = np.zeros((len(v), step), np.uint8)
        rec[:, :16] = np.ascontiguousarray(v).view(np.uint8).reshape(len(v), 16)
        vp.append(rec.reshape(-1))
        lp.append(np.ascontiguousarray(np.ascontiguousarray(l).view(np.uint8).reshape(len(l), 20)[:, :19]).reshape(-1))
    vd, va = W.lay_out(vp, 1)
    ld, la = W.lay_out(lp, 2)
    return (vd, va, np.array([len(v) for v, _ in frames], np.int32), step, (0, 4, 8, 12), ld, la, np.array([len(l) for _, l in frames], np.int32), 19)


def test_neighbour_slots_keep_what_they_held(M, synth):
    ctx = _ctx(M)
    try:
        for s in range(8):
            ctx.scan_upload(s, *_known(synth, s))
        ctx.extract(0, 8)
        before = [(_raw_words(ctx, s), ctx.slot_digest(s, 1)) for s in range(8)]
        assert len({d.tobytes() for _, d in before}) == 8
        rng = np.random.default_rng(7)
        for first, count in ((3, 2), (0, 1), (6, 2)):
            call = W.make_call(rng, [257, 64][:count], [63, 512][:count], 22, (0, 4, 8, 12), 19, first_residue=first)
            ctx.scan_upload_wire_batch(first, *call["args"])
            for s in range(8):
                (v, l), d = _raw_words(ctx, s), ctx.slot_digest(s, 1)
                if first <= s < first + count:
                    assert np.array_equal(v, call["velo"][s - first]) and np.array_equal(l, call["livox"][s - first])
                    before[s] = ((v, l), d)
                else:
                    assert np.array_equal(v, before[s][0][0]) and np.array_equal(l, before[s][0][1]) and np.array_equal(d, before[s][1]), (first, s)
    finally:
        ctx.close()


def test_extract_follows_without_synchronisation(M, synth):
    frames = [_known(synth, 20), _known(synth, 21)]
    args = _as_wire(frames)
    a, b = _ctx(M), _ctx(M)
    try:
        a.scan_upload_wire_batch(0, *args)
        a.extract(0, 2)      # (nothing synchronises between the two: the method above returns with the work enqueued)
        for i in range(2):
            _single(M, b, i, args, i)
        b.extract(0, 2)
        da, db = a.slot_digest(0, 2), b.slot_digest(0, 2)
        assert np.array_equal(da, db) and da[0].tobytes() != da[1].tobytes()
        info = a.scan_download(0)["info"]
        assert info.n_points > 300 and info.n_velo > 0 and info.n_points > info.n_velo
    finally:
        a.close()
        b.close()


def test_refusal_changes_nothing(M, synth):
    ctx = _ctx(M)
    try:
        for s in range(8):
            ctx.scan_upload(s, *_known(synth, s))
        before = [_raw_words(ctx, s) for s in range(8)]
        nl = [5, 6, 7, 8, 9, CAP + 1, 11, 12]     # frame 5 is one point over max_livox_points
        call = W.make_call(np.random.default_rng(8), [9] * 8, nl, 22, (0, 4, 8, 12), 19)
        with pytest.raises(M.MmlError) as e:
            ctx.scan_upload_wire_batch(0, *call["args"])
        assert e.value.code == M.MML_ERR_CAPACITY and "frame 5" in str(e.value) and "max_livox_points" in str(e.value)
        for s in range(8):
            v, l = _raw_words(ctx, s)
            assert v.shape == (CAP, 4) and l.shape == (CAP, 5)
            assert np.array_equal(v, before[s][0]) and np.array_equal(l, before[s][1])
        nl[5] = CAP                                # exactly at capacity: taken
        call = W.make_call(np.random.default_rng(8), [9] * 8, nl, 22, (0, 4, 8, 12), 19)
        ctx.scan_upload_wire_batch(0, *call["args"])
        assert np.array_equal(_raw_words(ctx, 5)[1], call["livox"][5])
    finally:
        ctx.close()


def test_stage_regrowth_and_many_tiles(M):
    """As tests/test_gpu_regrow.py: a context that saw a 64-point batch before the large one equals a fresh context that saw only
    the large one.  The large frames are a whole sweep of each sensor: about a hundred workgroup tiles per frame and sensor, at frame
    starts of different residues."""
    grown, fresh = M.Context(max_scans=2), M.Context(max_scans=2)
    try:
        nv, nl = min(28800, grown.cfg.max_velo_points), min(24000, grown.cfg.max_livox_points)
        assert nv > 4 * M.WIRE_TILE_POINTS and nl > 4 * M.WIRE_TILE_POINTS
        rng = np.random.default_rng(11)
        small = W.make_call(rng, [64, 64], [64, 64], 22, (0, 4, 8, 12), 19)
        large = W.make_call(rng, [nv, nv - 705], [nl - 833, nl], 22, (0, 4, 8, 12), 19, first_residue=3)
        grown.scan_upload_wire_batch(0, *small["args"])
        for c in (grown, fresh):
            c.scan_upload_wire_batch(0, *large["args"])
        for s in range(2):
            gv, gl = _raw_words(grown, s)
            fv, fl = _raw_words(fresh, s)
            assert np.array_equal(gv, fv) and np.array_equal(gl, fl)
            assert np.array_equal(fv, large["velo"][s]) and np.array_equal(fl, large["livox"][s])
    finally:
        grown.close()
        fresh.close()


def test_cpp_adapter_makes_the_same_call(M, synth, tmp_path):
    """feature_extraction::unionCloudWire, compiled against mmloam_adapter.hpp, against the ctypes calls on the same messages"""
    import subprocess
    from test_wire_batch_host import build_adapter_probe
    exe = tmp_path / "wire_batch_probe"
    build_adapter_probe(exe)
    vd, va, nv, step, offs, ld, la, nl, rec = args = _as_wire([_known(synth, 22), _known(synth, 23)])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([2, 1, 4, CAP, CAP, step, *offs, rec], "<i4").tobytes() + np.array([len(vd), len(ld)], "<i8").tobytes())
        f.write(va.astype("<i8").tobytes() + nv.astype("<i4").tobytes() + la.astype("<i8").tobytes() + nl.astype("<i4").tobytes())
        f.write(vd.tobytes() + ld.tobytes())
    run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "WIRE_BATCH_PROBE_DONE" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    raw = open(tmp_path / "out.bin", "rb").read()
    assert len(raw) == 2 * 4 + 2 * 80
    c = M.Context(max_scans=4, max_velo_points=CAP, max_livox_points=CAP)
    try:
        c.scan_upload_wire_batch(1, *args)
        c.extract(1, 2)
        assert np.frombuffer(raw[:8], "<i4").tolist() == [c.scan_info(1).n_points, c.scan_info(2).n_points]
        assert raw[8:] == c.slot_digest(1, 2).tobytes()
    finally:
        c.close()
