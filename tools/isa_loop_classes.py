#!/usr/bin/env python3
"""CPU: static instruction census of a solve kernel's pass loop in a hipcc -save-temps .s file, by class -- VALU, packed
VALU, v_cndmask, v_readlane / v_writelane, SALU, s_cbranch, s_nop, scalar memory, LDS, vector memory, s_waitcnt -- for the
loop (every block the assembler marks "in Loop") and for the code before it.

    hipcc --offload-arch=gfx950 <the flags of dex_retargeting_amd/_build.py> -save-temps -c csrc/dexr_tip_inst.hip
    python tools/isa_loop_classes.py dexr_tip_inst-hip-amdgcn-amd-amdhsa-gfx950.s [kernel name substring]
"""
import re
import sys
from collections import Counter

CLASSES = ["VALU", "packed VALU", "v_cndmask", "v_readlane/writelane", "SALU", "s_cbranch", "s_nop", "SMEM", "LDS", "VMEM/atomics",
           "s_waitcnt", "total"]


def classify(op):
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "v_readlane/writelane"
    if op.startswith("v_pk_"):
        return "packed VALU"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith(("s_cbranch", "s_branch")):
        return "s_cbranch"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM/atomics"
    if op.startswith("s_"):
        return "SALU"
    return None


def census(path, want=""):
    out, name, in_loop, seen_loop = {}, None, False, False
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, in_loop, seen_loop = m.group(1), False, False
            out[name] = {"prologue": Counter(), "loop": Counter(), "after": Counter()}
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        if re.match(r"^\.LBB\d+_\d+:", line) or re.match(r"^; %bb\.\d+:", line):
            in_loop = "in Loop" in line or "Loop Header" in line
            seen_loop = seen_loop or in_loop
            continue
        if "in Loop" in line or "Loop Header" in line:  # (the comment may sit on the line after the label)
            in_loop = seen_loop = True
            continue
        m = re.match(r"^\t([a-z_0-9]+)", line)
        if not m:
            continue
        c = classify(m.group(1))
        if c:
            part = "loop" if in_loop else ("after" if seen_loop else "prologue")
            out[name][part][c] += 1
            out[name][part]["total"] += 1
    return {k: v for k, v in out.items() if want in k and v["loop"]["total"]}


if __name__ == "__main__":
    for kname, parts in census(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "").items():
        print(f"# {kname}")
        print(f"{'class':24s} {'before loop':>12s} {'pass loop':>10s} {'between / after':>16s}")
        for c in CLASSES:
            print(f"{c:24s} {parts['prologue'][c]:12d} {parts['loop'][c]:10d} {parts['after'][c]:16d}")
