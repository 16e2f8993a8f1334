#!/usr/bin/env python3
"""Static VALU count of the EMIT path of a sort kernel in an ISA listing (.s from hipcc -S --cuda-device-only with the Makefile's
flags for the translation unit): the blocks from the 64-byte record gather of an instance (the first block with three or more
global_load_dwordx4) to the stores of its stream entry (the next block with three or more global_store_dwordx4), inclusive —
record gather, slot arithmetic, footprint masks (tile_mask.h instance_row_mask) and the stream stores of one pass of 64
instances.  Instructions are counted by role and priced with the issue costs of tools/isa_loop.py (profiles/r02/valu_rates_clock.txt);
every block counts once, i.e. a pass that takes every row branch.

    tools/isa_emit.py file.s <kernel-name-substring>"""
import re
import sys

from isa_loop import blocks, cost

ROLES = [("transcendental", r"v_(exp|rcp|rsq|log|sqrt)_f32"), ("compare", r"v_cmp"), ("select", r"v_cndmask"),
         ("fma/med3", r"v_(fma|mad|fmac|med3|min3|max3)_"), ("other VALU", r"v_")]


def role(line):
    for name, pat in ROLES:
        if re.match(pat, line):
            return name
    return None


def emit_region(path, kernel):
    bl = list(blocks(path, kernel))
    start = next(i for i, (_, b) in enumerate(bl) if sum(l.startswith("global_load_dwordx4") for l in b) >= 3)
    end = next(i for i in range(start, len(bl)) if sum(l.startswith("global_store_dwordx4") for l in bl[i][1]) >= 3)
    return bl[start:end + 1]


if __name__ == "__main__":
    region = emit_region(sys.argv[1], sys.argv[2])
    total = {name: 0 for name, _ in ROLES}
    cycles, branches, nblocks = 0.0, 0, 0
    for name, b in region:
        valu = [l for l in b if l.startswith("v_")]
        if not b:
            continue
        nblocks += 1
        for l in valu:
            total[role(l)] += 1
        cycles += sum(cost(l) for l in valu)
        branches += sum(l.startswith(("s_cbranch", "s_and_saveexec", "s_or_saveexec")) for l in b)
    n = sum(total.values())
    print(f"emit path: {nblocks} blocks, {n} VALU, {cycles:.0f} VALU issue cycles, {branches} saveexec / branch instructions")
    print("   " + ", ".join(f"{k} {v}" for k, v in total.items()))
