#!/usr/bin/env python3
"""ISA line and scratch-instruction counts of the radiance and probe kernels, from `hipcc -S` with the build's flags (no GPU needed).

usage: scripts/probe_isa.py [unit.hip ...]      default: rtw_radiance.hip rtw_probe.hip rtw_probe_sh.hip rtw_view.hip of raytracing_weekend_amd/csrc
Prints one line per kernel: ISA lines (instructions: lines that are neither labels, directives nor comments), scratch_ instructions,
and the VGPR / scratch / static LDS figures of the kernel's .amdhsa block. profiles/probe_rates.txt keeps the output of the parent's
rtw_radiance.hip beside this tree's, profiles/probe_sh_rates.txt the seven older kernels' beside k_probe_sh's, profiles/view_rates.txt
the thirteen older instantiations of the shared body in the parent and in this tree, beside k_view's. A unit given by path is compiled
where it lies, so a parent checkout's units are listed by naming them."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def counts(unit):
    flags = entry.unit_flags(os.path.basename(unit), next((extra for u, _, extra in entry.UNITS if u == os.path.basename(unit)), []))
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.check_call([entry.HIPCC] + flags + ["--cuda-device-only", "-S", "-o", out, unit])
        text = open(out).read()
    rows = []
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", text, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        code = body.split(".amdhsa_kernel")[0]
        inst = [ln for ln in code.splitlines() if ln.strip() and not ln.strip().startswith((";", ".", "//")) and not ln.rstrip().endswith(":")]
        scratch = sum(1 for ln in inst if ln.split()[0].startswith("scratch_"))
        vgpr = re.search(r"\.amdhsa_next_free_vgpr (\d+)", body)
        priv = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        lds = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body)
        demangled = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
        rows.append((demangled, len(inst), scratch, int(vgpr.group(1)) if vgpr else -1, int(priv.group(1)) if priv else -1,
                     int(lds.group(1)) if lds else -1))
    return rows


if __name__ == "__main__":
    units = sys.argv[1:] or [os.path.join(entry.CSRC, u) for u in ("rtw_radiance.hip", "rtw_probe.hip", "rtw_probe_sh.hip", "rtw_view.hip")]
    for u in units:
        print(f"# {os.path.basename(u)}")
        for name, n, scratch, vgpr, priv, lds in counts(u):
            print(f"{name:64s} {n:7d} ISA lines  {scratch:4d} scratch instructions  next_free_vgpr {vgpr:4d}  scratch bytes {priv:5d}  static LDS {lds:6d}")
