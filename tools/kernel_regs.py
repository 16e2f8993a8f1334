#!/usr/bin/env python3
"""Register / scratch budget of every kernel of a hipcc -save-temps assembly file:
  hipcc ... -save-temps=obj -c x.hip -o /tmp/x.o ; tools/kernel_regs.py /tmp/x-hip-amdgcn-amd-amdhsa-gfx950.s [filter]
Prints kernel (demangled head), VGPRs, AGPRs, bytes of scratch, the waves per SIMD the unified 512-register file allows, the
bytes of static LDS and the static instruction count (instruction lines of the kernel's body)."""
import re
import subprocess
import sys

text = open(sys.argv[1]).read()
flt = sys.argv[2] if len(sys.argv) > 2 else ""
vals = {}
for m in re.finditer(r"\.set (\S+)\.(num_vgpr|num_agpr|private_seg_size), (\d+)", text):
    vals.setdefault(m.group(1), {})[m.group(2)] = int(m.group(3))
for m in re.finditer(r"\.amdhsa_kernel (\S+)\n\s*\.amdhsa_group_segment_fixed_size (\d+)", text):
    vals.setdefault(m.group(1), {})["lds"] = int(m.group(2))
for m in re.finditer(r"^(\S+):[^\n]*\n(.*?)^\t\.amdhsa_kernel \1$", text, re.M | re.S):
    vals.setdefault(m.group(1), {})["insts"] = len(re.findall(r"^\t[a-z]", m.group(2), re.M))
for name, v in vals.items():
    if "num_vgpr" not in v or flt not in name:
        continue
    dem = name
    for filt in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            dem = subprocess.run([filt, name], capture_output=True, text=True).stdout.strip() or name
            break
        except OSError:
            pass
    dem = re.sub(r"\(anonymous namespace\)::", "", dem).split("(")[0]
    vg, ag = v["num_vgpr"], v.get("num_agpr", 0)
    tot = ((vg + 3) // 4 * 4 if ag else vg) + ag
    tot8 = (tot + 7) // 8 * 8
    print(f"{dem[:90]:90s} vgpr {vg:3d} agpr {ag:3d} scratch {v.get('private_seg_size', 0):4d} B  waves/SIMD {min(8, 512 // max(tot8, 1))}  lds {v.get('lds', 0):6d} B  insts {v.get('insts', 0):5d}")
