#!/usr/bin/env python3
"""Instruction streams of two builds, kernel by kernel:
  hipcc <flags> --cuda-device-only -S x.hip -o x.s
  tools/isa_streams.py before.s [more.s ...] -- after.s [more.s ...]
A kernel's stream: the lines between `<sym>:` and `.amdhsa_kernel <sym>`, `;` comments dropped, the function numbers of
`.LBB<n>_` and `.Ltmp<n>` normalised, instruction lines only.  Prints, per kernel symbol, "identical" or the difference by
mnemonic.  Exit status 1 when a stream differs or the two sides do not hold the same set of kernel symbols."""
import collections
import re
import sys


def streams(paths):
    out = {}
    for path in paths:
        text = open(path).read()
        for m in re.finditer(r"^(\S+):[^\n]*\n(.*?)^\t\.amdhsa_kernel \1$", text, re.M | re.S):
            body = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\.Ltmp\d+", ".Ltmp", re.sub(r";.*", "", m.group(2))))
            assert m.group(1) not in out, "kernel symbol twice on one side: " + m.group(1)
            out[m.group(1)] = [" ".join(line.split()) for line in body.split("\n") if re.match(r"\t[a-z]", line)]
    return out


cut = sys.argv.index("--")
a, b = streams(sys.argv[1:cut]), streams(sys.argv[cut + 1:])
bad = 0
for sym in sorted(set(a) | set(b)):
    if sym not in a or sym not in b:
        print(f"{sym}: only {'before' if sym in a else 'after'} the --")
        bad += 1
    elif a[sym] == b[sym]:
        print(f"{sym}: identical ({len(a[sym])} instructions)")
    else:
        ca, cb = (collections.Counter(line.split()[0] for line in s[sym]) for s in (a, b))
        moved = ", ".join(f"{k} {ca[k]} -> {cb[k]}" for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k])
        print(f"{sym}: DIFFERENT, {len(a[sym])} -> {len(b[sym])} instructions: {moved or 'same mnemonics, other order or operands'}")
        bad += 1
print(f"{len(a)} kernels before, {len(b)} after, {bad} not identical")
sys.exit(1 if bad else 0)
