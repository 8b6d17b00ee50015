"""Phase clocks of the hot kernels (csrc/phase_clock.h): cycles per phase of one watched workgroup or wavefront, from a library built
with the family's flag -- e.g. make BUILD=build_t OUT=../libmmloam_hip_t.so EXTRA=-DMML_ST_TIMING=3 in csrc, then
  MML_LIB_PATH=multi-modal-loam_amd/libmmloam_hip_t.so python tools/phases.py <family> [reps]
Families: op st sel sp vx sv svw (the table below says which kernel, which flag and which workload)."""
import ctypes as C
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


# ---- workloads: reset() zeroes the clocks at the point from which the launches count; the return value is the timed repetitions ----
def _batch_context(M):
    synth = importlib.import_module("multi-modal-loam_amd.synth")
    ctx = M.Context(max_scans=1024, device=0)
    scans = [(synth.velo_scan(k), synth.livox_scan(k)) for k in range(8)]
    for s in range(1024):
        ctx.scan_upload(s, *scans[s % 8])
    ctx.synchronize()
    return ctx


def extract(M, reps, reset):  # the feature stage over 1024 slots
    ctx = _batch_context(M)
    for _ in range(2):
        ctx.extract(0, 1024)
    ctx.synchronize()
    reset()
    for _ in range(reps):
        ctx.extract(0, 1024)
    ctx.synchronize()
    return reps


def downsample(M, reps, reset):  # the voxel filter over 1024 extracted slots
    import numpy as np
    ctx = _batch_context(M)
    ctx.extract(0, 1024)
    ctx.undistort(0, 1024, np.tile(np.eye(3).reshape(1, 9), (1024, 1)), np.zeros((1024, 3)))
    ctx.downsample(0, 1024)
    ctx.synchronize()
    reset()
    for _ in range(reps):
        ctx.downsample(0, 1024)
    ctx.synchronize()
    return reps


def bench_full(M, reps, reset):  # the default bench workload: the batch solves (k_solve)
    sys.argv = ["bench.py", "--full", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0", "--kernel-steps", "2"]
    import bench
    import torch
    torch.cuda.init()  # (torch's HIP runtime first, as in bench.py: the library is loaded next to it)
    reset()
    bench.main()
    return 1


def live_step(M, reps, reset):  # the live path, one slot per mml_step call: MML_SOLVE_WIDE=1 k_solve_wide, =0 k_solve<true>
    import stage_probe
    reset()
    stage_probe.main(1, reps)
    return reps


# ---- the table.  A report is a list of parts (title, unit, per, rows, shares):
#   per     None: the rows are divided by the timed repetitions; (family, slot): by that counter, and the part is left out when it is 0
#   rows    (family, slot, name): a slot of accumulated cycles (or a counter)
#   shares  the rows are also shown as shares of their sum
# "stamps" in place of per: the rows are absolute clock values of the last pass, shown as the difference to the row before
K_SOLVE = [("sv", 0, "set-up + first evaluation"), ("sv", 1, "propose (wave 0) + barrier"), ("sv", 2, "factor pass (thread 0)"),
           ("sv", 3, "block reduction"), ("sv", 4, "decide (wave 0) + barrier")]
FAMILIES = {
    "op": dict(flag="MML_OP_TIMING=<block>", workload=extract, reps=5, report=[
        ("k_assign_onepass_s<0>, second wavefront of one block", "clock64 ticks per launch", None, [
            ("op", 0, "records requested, point count read, counters zeroed"), ("op", 1, "barrier 1"),
            ("op", 2, "evaluate 8 points (waits for its records)"), ("op", 3, "barrier 2"), ("op", 4, "scan over groups"),
            ("op", 5, "barrier 3"), ("op", 6, "barrier 4 (wavefront 0: publish, look back)"), ("op", 7, "16-byte stores + LDS rows"),
            ("op", 8, "barrier 5"), ("op", 9, "row stores + drain")], True),
        ("first wavefront", "clock64 ticks per launch", None, [
            ("op", 10, "from the kernel's start to its serial section"), ("op", 11, "publish + look-back poll"),
            ("op", 12, "reduce + block record")], False)]),
    "st": dict(flag="MML_ST_TIMING=<line>", workload=extract, reps=5, report=[
        ("k_stencil phases (one wavefront)", "clock64 ticks per launch", None, [
            ("st", 0, "wait-prev"), ("st", 1, "load+sq"), ("st", 2, "rounds"), ("st", 3, "walk"), ("st", 4, "list+c150"),
            ("st", 5, "write")], True)]),
    "sel": dict(flag="MML_SEL_TIMING=<line>", workload=extract, reps=5, report=[
        ("k_select phases (thread 0 of one line, its last launch)", "clock64 ticks between the marks", "stamps", [
            ("sel", 0, "(start)"), ("sel", 1, "load the line's attributes and keys"), ("sel", 2, "phase 0: per-point record"),
            ("sel", 3, "phase 1: who can suppress me"), ("sel", 4, "dependency rounds"), ("sel", 5, "phase 2: value held, later marks"),
            ("sel", 6, "phase 3: :521-539 in closed form"), ("sel", 7, "(a2) reflect before curvature visit (uncached form)"),
            ("sel", 8, "(a2) + (b) eff3 / G bits"), ("sel", 10, "(phase 4 is k_stencil's)"), ("sel", 11, "phase 5: final value, emit, labels")],
         True),
        ("k_select counters", "per extract call", None, [("sel", 20, "dependency rounds (all launches)")], False)]),
    "sp": dict(flag="MML_SP_TIMING=<line>", workload=extract, reps=5, report=[
        ("k_select_part phases (one wavefront)", "clock64 ticks per launch", None, [
            ("sp", 0, "A planes"), ("sp", 1, "B extract+static"), ("sp", 2, "B rounds"), ("sp", 3, "B refl top3"), ("sp", 4, "B ranks"),
            ("sp", 5, "B minE/minG"), ("sp", 6, "B final+scatter"), ("sp", 7, "C flags")], True)]),
    "vx": dict(flag="MML_VX_TIMING=<kind: 0 corner | 1 surf>", workload=downsample, reps=5, report=[
        ("k_voxel<512> phases (second wavefront of one workgroup)", "clock64 ticks per launch", None, [
            ("vx", 4, "list + point gathers, min / max"), ("vx", 5, "min / max reduction (1 barrier)"), ("vx", 6, "voxel keys"),
            ("vx", 7, "radix sort"), ("vx", 0, "(return)"), ("vx", 1, "centroid: gathers to LDS, heads (per chunk)"),
            ("vx", 2, "centroid: per-voxel sums"), ("vx", 3, "centroid: barriers")], True)]),
    "sv": dict(flag="MML_SV_TIMING=<problem>", workload=bench_full, reps=1, report=[
        ("k_solve phases (one workgroup)", "clock64 ticks per launch", ("sv", 7), K_SOLVE, True),
        ("inside the proposal (first wavefront)", "clock64 ticks per launch", ("sv", 7), [
            ("sv", 8, "diag / gradient / alpha"), ("sv", 9, "Cholesky"), ("sv", 10, "substitutions"), ("sv", 11, "dogleg"),
            ("sv", 12, "model change")], False)]),
    "svw": dict(flag="MML_SV_TIMING=0", workload=live_step, reps=200, report=[
        ("k_solve_wide", "clock64 ticks per launch", ("svw", 6), [
            ("svw", 5, "cycles, start to end"), ("svw", 4, "passes"), ("sv", 1, "proposal + barrier"),
            ("sv", 4, "accept / reject + barrier"), ("sv", 0, "everything else")], False),
        ("k_solve_wide's factor pass (thread 0)", "clock64 ticks per pass", ("svw", 4), [
            ("svw", 0, "rows (thread 0)"), ("svw", 1, "wait at the barrier"), ("svw", 2, "sums"), ("svw", 3, "tree + final barriers")], False),
        ("k_solve<true>", "clock64 ticks per launch", ("sv", 7), K_SOLVE, True)]),
}


def main(family, reps=None):
    M = importlib.import_module("multi-modal-loam_amd")
    spec = FAMILIES[family]
    read = sorted({fam for part in spec["report"] for fam, _, _ in part[3]})
    slots = {fam: (C.c_ulonglong * 64)() for fam in read}

    def clocks(reset):
        for fam in read:
            rc = M.phase_clocks(fam, slots[fam], reset)
            if rc == M.PHASE_CLOCKS_NOT_BUILT:
                sys.exit("this library has no '%s' phase clocks: build it with -D%s and name it in $MML_LIB_PATH" % (fam, spec["flag"]))
            if rc < 0:
                sys.exit("mml_debug_phase_clocks('%s'): %d" % (fam, rc))

    n = spec["workload"](M, reps or spec["reps"], lambda: clocks(True))
    clocks(False)
    for title, unit, per, rows, shares in spec["report"]:
        vals = [int(slots[fam][slot]) for fam, slot, _ in rows]
        if per == "stamps":  # differences between the marks the line passed (a mark of the other form of the kernel stays 0)
            passed = [(v, name) for v, (_, _, name) in zip(vals, rows) if v >= vals[0]]
            vals, names, div = [b[0] - a[0] for a, b in zip(passed, passed[1:])], [name for _, name in passed[1:]], 1
        else:
            names, div = [name for _, _, name in rows], n if per is None else int(slots[per[0]][per[1]])
        if div == 0:
            continue
        tot = sum(vals)
        print("%s, %s%s%s" % (title, unit, "" if per in (None, "stamps") else " (%d of them)" % div,
                                            ", total %d" % (tot // div) if shares else ""))
        for v, name in zip(vals, names):
            print("  %-54s %9d%s" % (name, v // div, "  %5.1f%%" % (100.0 * v / max(tot, 1)) if shares else ""))


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in FAMILIES:
        sys.exit(__doc__)
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else None)
