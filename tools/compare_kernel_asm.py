#!/usr/bin/env python3
"""Two device assembly listings of one source file (hipcc --offload-arch=gfx950 --offload-device-only -S, the Makefile's flags), kernel by
kernel: registers, LDS and scratch from the metadata of each kernel, and whether the instruction streams are the same (labels, comments
and directives stripped, block numbers kept).
    python tools/compare_kernel_asm.py parent.s change.s [kernel whose instructions may differ ...]
Build-machine tool: needs no GPU."""
import re
import subprocess
import sys


def kernels(path):
    """{demangled name: (metadata dict, [instructions])}"""
    out, name, body = {}, None, []
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        d = dict(re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|group_segment_fixed_size|private_segment_fixed_size) (\d+)", m.group(2)))
        meta[m.group(1)] = d
    for line in text.split("\n"):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if m and m.group(1) in meta:
            name, body = m.group(1), []
            out[name] = body
            continue
        if name is None:
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            name = None
            continue
        if not s or s.startswith(".") and not s.startswith(".LBB") or s.endswith(":") and not s.startswith(".LBB"):
            continue
        body.append(s)
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.split("\n")
    res = {}
    for mangled, nice in zip(out, names):
        nice = nice.split("(")[0].replace("void ", "").replace("pope::", "")
        res[nice] = (meta[mangled], out[mangled])
    return res


def resources(m):
    vgpr, acc = int(m["next_free_vgpr"]), int(m.get("accum_offset", 0))
    arch = min(vgpr, acc) if acc else vgpr          # unified file: architectural VGPRs below accum_offset, AGPRs above
    return "%d+%d/%s/%s/%s" % (arch, vgpr - arch, m["next_free_sgpr"], m["group_segment_fixed_size"], m["private_segment_fixed_size"])


if __name__ == "__main__":
    parent, change, allowed = kernels(sys.argv[1]), kernels(sys.argv[2]), set(sys.argv[3:])
    print("kernels: parent %d, change %d; same set: %s\n" % (len(parent), len(change), sorted(parent) == sorted(change)))
    print("%-28s %-26s %-26s %s" % ("kernel", "parent v+a/s/lds/scr", "change v+a/s/lds/scr", "instructions"))
    bad = 0
    for k in sorted(set(parent) | set(change)):
        if k not in parent or k not in change:
            print("%-28s only in %s" % (k, "parent" if k in parent else "change"))
            bad += 1
            continue
        (pm, pi), (cm, ci) = parent[k], change[k]
        same = pi == ci
        note = "identical (%d)" % len(pi) if same else "DIFFER (%d -> %d)%s" % (len(pi), len(ci), ", allowed" if k in allowed else "")
        if resources(pm) != resources(cm) or (not same and k not in allowed):
            bad += 1
        print("%-28s %-26s %-26s %s" % (k, resources(pm), resources(cm), note))
    print("\nkernels whose resources differ, or whose instructions differ without being allowed to: %d" % bad)
