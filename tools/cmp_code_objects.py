#!/usr/bin/env python3
"""Developer check for refactors of host code: python3 tools/cmp_code_objects.py parent.o branch.o -- compares the gfx950 code objects of two builds of one translation unit, kernel by kernel:
the set of symbols, every symbol's size, every kernel's metadata (registers, LDS, scratch, spills, kernarg) and code bytes.
A side may be several objects joined by commas (a unit that was split: parent.o branch.o,branch_new.o): their union is compared."""
import re, subprocess, sys, os, tempfile
B = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "")
def load(o, tag):
    d = tempfile.mkdtemp()
    fb, co = os.path.join(d, "fb"), os.path.join(d, "co")
    subprocess.check_call([B + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, o])
    subprocess.check_call([B + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co])
    syms = {}
    for l in subprocess.check_output([B + "llvm-readelf", "-s", "--wide", co], text=True).splitlines():
        f = l.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and not f[7].startswith("__hip_cuid_"):
            syms[f[7]] = (f[3], int(f[2]), int(f[1], 16))
    text = None
    for l in subprocess.check_output([B + "llvm-readelf", "-S", "--wide", co], text=True).splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", l)
        if m: text = (int(m.group(1), 16), int(m.group(2), 16))
    raw = open(co, "rb").read()
    code = {n: raw[text[1] + a - text[0]: text[1] + a - text[0] + sz] for n, (t, sz, a) in syms.items() if t == "FUNC"}
    meta, cur = {}, None
    for l in subprocess.check_output([B + "llvm-readelf", "--notes", co], text=True).splitlines():
        m = re.match(r"\s*(?:- )?\.(\w+):\s*(.*)$", l)
        if not m: continue
        k, v = m.groups()
        if l.lstrip().startswith("- .agpr_count"): cur = {}
        if cur is not None and k in ("agpr_count", "vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "sgpr_spill_count",
                                     "vgpr_spill_count", "kernarg_segment_size", "max_flat_workgroup_size", "uses_dynamic_stack", "wavefront_size"):
            cur[k] = v
        if cur is not None and k == "name" and v.startswith("_Z"): meta[v] = cur
    return syms, code, meta
def side(arg, tag):
    syms, code, meta = {}, {}, {}
    for o in arg.split(","):
        for whole, part in zip((syms, code, meta), load(o, tag)): whole.update(part)
    return syms, code, meta
a, b = side(sys.argv[1], "a"), side(sys.argv[2], "b")
bad = 0
for n in sorted(set(a[0]) | set(b[0])):
    if n not in a[0] or n not in b[0]: print("only on one side:", n); bad += 1
    elif a[0][n][:2] != b[0][n][:2]: print("size differs:", n, a[0][n][1], b[0][n][1]); bad += 1
for n in sorted(set(a[2]) | set(b[2])):
    if a[2].get(n) != b[2].get(n): print("metadata differs:", n, a[2].get(n), b[2].get(n)); bad += 1
same_code = sum(1 for n in a[1] if b[1].get(n) == a[1][n])
print("%d symbols, %d kernels with metadata, %d of %d functions with identical code bytes" % (len(a[0]), len(a[2]), same_code, len(a[1])))
print("no differences" if not bad else "%d DIFFERENCES" % bad)
sys.exit(1 if bad else 0)
