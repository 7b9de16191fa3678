#!/usr/bin/env python3
"""Static instruction counts of one kernel by class and basic block, from the assembly `make -C salt_amd/csrc asm` writes.

usage: isa_counts.py FILE.s KERNEL_SUBSTRING
Classes: VALU (v_*), SALU (s_* but waits, barriers, branches and nops), LDS (ds_*), VMEM (global_*, flat_*, buffer_*, scratch_*), SMEM
(scalar loads), BRANCH, WAIT (s_waitcnt, s_barrier, s_nop).  A block starts at a label; the counts say nothing about trip counts."""
import re
import sys


def classify(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")):
        return "BRANCH"
    if op.startswith(("s_waitcnt", "s_barrier", "s_nop", "s_sleep")):
        return "WAIT"
    if op.startswith("s_"):
        return "SALU"
    return None


def main():
    path, name = sys.argv[1], sys.argv[2]
    classes = ("VALU", "SALU", "LDS", "VMEM", "SMEM", "BRANCH", "WAIT")
    blocks, cur, inside = [], None, False
    for line in open(path):
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        if m and not line.startswith("."):
            if inside:
                break
            inside = name in m.group(1)
            if inside:
                cur = [m.group(1)[:40], dict.fromkeys(classes, 0)]
                blocks.append(cur)
            continue
        if not inside:
            continue
        if m:
            cur = [m.group(1), dict.fromkeys(classes, 0)]
            blocks.append(cur)
            continue
        if ".end_amdhsa_kernel" in line or line.startswith("\t.section"):
            break
        t = line.split("//")[0].split(";")[0].split()
        if t and classify(t[0]):
            cur[1][classify(t[0])] += 1
    print("%-42s" % "block" + "".join("%8s" % c for c in classes))
    total = dict.fromkeys(classes, 0)
    for label, cnt in blocks:
        if any(cnt.values()):
            print("%-42s" % label + "".join("%8d" % cnt[c] for c in classes))
        for c in classes:
            total[c] += cnt[c]
    print("%-42s" % "total" + "".join("%8d" % total[c] for c in classes))


if __name__ == "__main__":
    main()
