#!/usr/bin/env python3
"""Are the kernels of two checkouts the same machine code? Every unit of __graft_entry__.UNITS is compiled with `hipcc -S` and
the build's flags (no GPU needed) in this tree and in another checkout - each by its own checkout's recipe - and every kernel is compared: instruction
count, next_free_vgpr, next_free_sgpr, scratch bytes, static LDS, and a hash of its instruction text (labels, directives and
comments left out).

usage: scripts/isa_compare.py OTHER_CHECKOUT [-j N]
Prints one line per kernel of the other checkout - "same" or what differs - then the kernels only this tree has, with their
figures. Exit status 1 if a kernel of the other checkout differs or is missing here. profiles/probe_adaptive_isa.txt keeps the
output for the parent of rtw_probe_adaptive."""
import concurrent.futures
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def recipe_of(root):
    """That checkout's own build recipe: its __graft_entry__ imported by path. -> (UNITS, flags of a unit)"""
    spec = importlib.util.spec_from_file_location("entry_" + hashlib.sha256(root.encode()).hexdigest()[:8], os.path.join(root, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if hasattr(mod, "UNITS"):
        return mod.UNITS, mod.unit_flags
    # a checkout from before UNITS: the list literal and the common flags cut out of build()'s text (they name UNIT_FLAGS and HIP_FLAGS)
    text = open(os.path.join(root, "__graft_entry__.py")).read()
    body = text[text.index("units = ["):text.index("cflags = ")]
    units = eval(body.split("=", 1)[1].strip(), {"UNIT_FLAGS": mod.UNIT_FLAGS})
    cflags = eval(text[text.index("cflags = "):].split("\n")[0].split("=", 1)[1], {"HIP_FLAGS": mod.HIP_FLAGS})
    return units, lambda unit, extra: cflags + extra + mod.UNIT_FLAGS.get(unit, [])


def kernels(root, flags_of, unit, obj, extra):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.check_call([entry.HIPCC] + flags_of(unit, extra) + ["--cuda-device-only", "-S", "-o", out,
                               os.path.join(root, "raytracing_weekend_amd", "csrc", unit)], stderr=subprocess.DEVNULL)
        text = open(out).read()
    rows = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*\.end_amdhsa_kernel", text, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        code = body.split(".amdhsa_kernel")[0]
        # (.LBB<function number>_<block>: the number moves when a unit gains a kernel before this one)
        inst = [re.sub(r"\.LBB\d+_", ".LBB_", " ".join(ln.split(";")[0].split())) for ln in code.splitlines()
                if ln.strip() and not ln.strip().startswith((";", ".", "//")) and not ln.rstrip().endswith(":")]

        def field(key):
            f = re.search(r"\.amdhsa_" + key + r" (\d+)", body)
            return int(f.group(1)) if f else -1
        rows[(obj, name)] = (len(inst), field("next_free_vgpr"), field("next_free_sgpr"), field("private_segment_fixed_size"),
                             field("group_segment_fixed_size"), hashlib.sha256("\n".join(inst).encode()).hexdigest()[:16])
    return rows


def all_kernels(root, jobs):
    out = {}
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        units, flags_of = recipe_of(root)
        for rows in ex.map(lambda u: kernels(root, flags_of, *u), units):
            out.update(rows)
    return out


def demangle(name):
    return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]


if __name__ == "__main__":
    other = os.path.abspath(sys.argv[1])
    jobs = int(sys.argv[sys.argv.index("-j") + 1]) if "-j" in sys.argv else 8
    theirs, ours = all_kernels(other, jobs), all_kernels(ROOT, jobs)
    cols = ("instructions", "next_free_vgpr", "next_free_sgpr", "scratch bytes", "static LDS", "text hash")
    bad = 0
    print(f"# {len(theirs)} kernels in the other checkout, {len(ours)} here; per kernel: {', '.join(cols)}")
    for key in sorted(theirs):
        a, b = theirs[key], ours.get(key)
        label = f"{key[0]:24s} {demangle(key[1]):72s}"
        if b is None:
            bad += 1
            print(f"{label} MISSING here")
        elif a == b:
            print(f"{label} same  {a[0]:6d} {a[1]:4d} {a[2]:4d} {a[3]:5d} {a[4]:6d} {a[5]}")
        else:
            bad += 1
            print(f"{label} DIFFERS  " + "; ".join(f"{c}: {x} -> {y}" for c, x, y in zip(cols, a, b) if x != y))
    print("# kernels only this tree has")
    for key in sorted(set(ours) - set(theirs)):
        b = ours[key]
        print(f"{key[0]:24s} {demangle(key[1]):72s} new   {b[0]:6d} {b[1]:4d} {b[2]:4d} {b[3]:5d} {b[4]:6d} {b[5]}")
    print(f"# {len(theirs) - bad} of {len(theirs)} kernels of the other checkout are the same here, {bad} differ or are missing")
    sys.exit(1 if bad else 0)
