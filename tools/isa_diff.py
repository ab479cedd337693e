"""Kernel by kernel, are two AMDGPU assembly listings (hipcc -S --cuda-device-only) the same instructions?
Labels are normalised; comments and directives are dropped.  Prints, per kernel of either listing, "identical" or "differs"
with both instruction counts and both register / spill lines (the figures of tools/isa_stats.py).
usage: python tools/isa_diff.py old.s new.s [--rename REGEX REPL]   (REGEX -> REPL on the old listing's demangled names)"""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"- \.agpr_count.*?\.wavefront_size", text, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)
        meta[re.search(r"\.name:\s+(\S+)", blk).group(1)] = "vgpr %s agpr %s sgpr %s  vgpr_spill %s sgpr_spill %s  lds %s scratch %s" % (
            g("vgpr_count"), g("agpr_count"), g("sgpr_count"), g("vgpr_spill_count"), g("sgpr_spill_count"),
            g("group_segment_fixed_size"), g("private_segment_fixed_size"))
    names = list(meta)
    nice = names
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            nice = subprocess.run([tool], input="\n".join(names), stdout=subprocess.PIPE, universal_newlines=True).stdout.split("\n")
            break
        except OSError:
            pass
    out = {}
    for name, pretty in zip(names, nice):
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index("\n.Lfunc_end")]
        ins = []
        for line in body.split("\n")[2:]:
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not line.endswith(":")):
                continue
            ins.append(re.sub(r"\.L(BB|tmp|func_\w+?)\d+", r".L\1", line))
        out[pretty.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").strip()] = (ins, meta[name])
    return out


args = sys.argv[1:]
old, new = kernels(args[0]), kernels(args[1])
if len(args) > 2 and args[2] == "--rename":
    old = {re.sub(args[3], args[4], k): v for k, v in old.items()}
same = 0
for k in sorted(set(old) | set(new)):
    if k not in old or k not in new:
        print("%s\n    only in the %s listing: %d instructions, %s" % ((k, "new") + (len(new[k][0]), new[k][1]) if k in new
                                                                        else (k, "old") + (len(old[k][0]), old[k][1])))
        continue
    verdict = "identical" if old[k][0] == new[k][0] else "differs"
    same += verdict == "identical"
    print("%s\n    %s: %d -> %d instructions\n    old %s\n    new %s" % (k, verdict, len(old[k][0]), len(new[k][0]), old[k][1], new[k][1]))
print("%d kernels identical, %d differ or have no counterpart" % (same, len(set(old) | set(new)) - same))
