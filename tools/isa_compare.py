#!/usr/bin/env python3
"""Compares the gfx950 ISA of the association kernels between two builds of csrc/map_assoc.hip.

    hipcc <the Makefile's FLAGS> -save-temps -c map_assoc.hip      (once in each tree)
    python tools/isa_compare.py OLD/map_assoc-hip-amdgcn-amd-amdhsa-gfx950.s NEW/map_assoc-hip-amdgcn-amd-amdhsa-gfx950.s
    python tools/isa_compare.py OLD/capi-hip-amdgcn-amd-amdhsa-gfx950.s NEW/capi-hip-amdgcn-amd-amdhsa-gfx950.s k_encode,k_fused
        (a third argument: the name prefixes of the kernels to compare, for another translation unit)

Kernels are matched by their demangled base name and, for templates, their arguments without the trailing `false` of the
unbanked instantiations (a build from before the banked forms has no such argument; the `true` ones are listed, not compared).
Compared per kernel: the instruction text between the
kernel's label and its s_endpgm with symbol names removed, and the register / scratch / LDS figures of its .amdhsa block.
Prints one line per kernel and exits 1 when a pair differs."""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+|k_\w+):[^\n]*\n(.*?)^\s*s_endpgm", text, re.S | re.M):   # (k_...: an extern "C" kernel)
        name, body = m.group(1), m.group(2)
        meta = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), text, re.S)
        if not meta:
            continue
        lines = [re.sub(r"\s*;.*$", "", l).strip() for l in body.splitlines()]
        lines = [l for l in lines if l and not l.startswith((".", ";"))]
        lines = [re.sub(r"_Z\w+", "SYM", l) for l in lines]
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in lines]
        keep = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size",
                "kernarg_size")
        figures = {k: v for k, v in re.findall(r"\.amdhsa_(\w+) (\S+)", meta.group(1)) if k in keep}
        out[name] = (lines, figures)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def key(dem, new):
    """k_associate_hard<4>(AssocParams, int) and k_associate_hard<4, false>(AssocArgs<false>, int) -> ('k_associate_hard', '4')"""
    m = re.search(r"(k_\w+)(?:<([^>]*)>)?(?:\(|$)", dem)
    if not m or not m.group(1).startswith(PREFIXES):
        return None
    args = [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
    if args and args[-1] in ("false", "true"):           # (an old build from before the banked forms has no such argument)
        if args[-1] == "true":
            return None
        args = args[:-1]
    return (m.group(1), ",".join(args))


PREFIXES = ("k_associate", "k_assoc_prefix", "k_knn5")


def main():
    global PREFIXES
    if len(sys.argv) > 3:   # another translation unit's kernels: a comma-separated list of name prefixes, e.g. k_encode
        PREFIXES = tuple(sys.argv[3].split(","))
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    dold, dnew = demangle(list(old)), demangle(list(new))
    kold = {key(dold[n], False): n for n in old if key(dold[n], False)}
    knew = {key(dnew[n], True): n for n in new if key(dnew[n], True)}
    bad = 0
    for k in sorted(kold):
        if k not in knew:
            print("%-28s missing in the new build" % (k[0] + ("<%s>" % k[1] if k[1] else "")))
            bad += 1
            continue
        (lo, fo), (ln, fn) = old[kold[k]], new[knew[k]]
        same = lo == ln and fo == fn
        bad += 0 if same else 1
        print("%-28s %5d instructions  vgpr %s sgpr %s scratch %s  %s" % (k[0] + ("<%s>" % k[1] if k[1] else ""), len(ln), fn.get("next_free_vgpr"),
                                                                        fn.get("next_free_sgpr"), fn.get("private_segment_fixed_size"),
                                                                        "IDENTICAL" if same else "DIFFERENT (old: %d instructions, %s)" % (len(lo), fo)))
    banked = [n for n in new if re.search(r"<(?:\d+, )?true>", dnew[n])]
    for n in sorted(banked, key=lambda n: dnew[n]):
        l, f = new[n]
        print("%-28s %5d instructions  vgpr %s sgpr %s scratch %s  (banked form)" % (re.search(r"k_\w+(?:<[^>]*>)?", dnew[n]).group(0), len(l),
                                                                                   f.get("next_free_vgpr"), f.get("next_free_sgpr"),
                                                                                   f.get("private_segment_fixed_size")))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
