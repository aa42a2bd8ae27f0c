#!/usr/bin/env python3
"""Which kernels differ between two device assembly files of the library (before / after a change that should not touch them)?
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC --cuda-device-only -S csrc/ssg_hip.hip -o <file.s>
usage: kernel_diff.py <before.s> <after.s> [before_name=after_name ...]
A kernel's text is everything from its label to the end of its .amdhsa_kernel block (instructions, register / LDS / scratch / kernarg
figures).  Kernels are matched by demangled name without the `ssg::` namespace; a renamed kernel is matched by a `before=after` pair of
names up to the parameter list (e.g. `bitonic_local_dev_kernel=bitonic_local_kernel<true>`).  Inside the text every mangled symbol
the function number of every local label and runs of blanks are normalised.  Prints the kernels that differ (with both sets of figures, as
kernel_regs.py prints them) and the ones only one file has; exit status 1 when there are any."""
import re
import shutil
import subprocess
import sys

CXXFILT = shutil.which("llvm-cxxfilt", path="/opt/rocm/lib/llvm/bin") or shutil.which("c++filt")


def kernels(path):
    txt = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M)
    plain = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    metas = {re.search(r"\.name:\s+(\S+)", blk)[1]: blk for blk in txt.split("  - .agpr_count:")[1:]}
    out = {}
    for sym, dem in zip(names, plain):
        a = txt.index("\n%s:" % sym)
        body = txt[a:txt.index(".end_amdhsa_kernel", a)]
        body = re.sub(r"[ \t]+", " ", re.sub(r"BB\d+_", "BB_", re.sub(r"_Z\w+", "SYM", body)))     # (comment columns shift with a label's width)
        meta = metas[sym]
        fig =" ".join("%s %s" % (k, re.search(r"\.%s:\s+(\S+)" % f, meta)[1]) for k, f in
                       (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("spill", "vgpr_spill_count"), ("scratch", "private_segment_fixed_size"),
                        ("lds", "group_segment_fixed_size"), ("kernarg", "kernarg_segment_size")))
        key = re.sub(r"^void ", "", dem).replace("ssg::", "")
        assert key not in out, key
        out[key] = (body, fig)
    return out


before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
for pair in sys.argv[3:]:
    old, new = pair.split("=")
    for k in [k for k in before if k.split("(")[0] == old]:
        new_keys = [c for c in after if c.split("(")[0] == new]
        assert len(new_keys) == 1, (pair, new_keys)
        before[new_keys[0] + "   [was " + old + "]"] = before.pop(k)
        after[new_keys[0] + "   [was " + old + "]"] = after.pop(new_keys[0])
same = [k for k in before if k in after and before[k][0] == after[k][0]]
differ = [k for k in before if k in after and before[k][0] != after[k][0]]
print("%d kernels before, %d after, %d identical" % (len(before), len(after), len(same)))
for k in differ:
    print("DIFFERS  %s\n   before: %s\n   after:  %s" % (k, before[k][1], after[k][1]))
for k in before:
    if k not in after:
        print("ONLY BEFORE  %s\n   %s" % (k, before[k][1]))
for k in after:
    if k not in before:
        print("ONLY AFTER   %s\n   %s" % (k, after[k][1]))
sys.exit(1 if differ or len(same) != len(before) or len(same) != len(after) else 0)
