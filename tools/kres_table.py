#!/usr/bin/env python3
"""Kernel resource table of one translation unit before / after a change that must not move its kernels.
Inputs per side: the host object hipcc wrote and the stderr of the same compile with -Rpass-analysis=kernel-resource-usage.
usage: python tools/kres_table.py LABEL old.o old.remarks new.o new.remarks [LABEL ...]   (five arguments per table)
Each of the four files may be a comma-separated list (a.o,b.o and a.remarks,b.remarks) when the kernels moved to another translation unit.
Columns: VGPRs / AGPRs / LDS bytes / scratch bytes per lane / occupancy (waves per SIMD) as old -> new where they differ, the code
size in bytes, and whether the kernel's instruction bytes are identical."""
import hashlib, os, re, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"
KEYS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("LDS", "LDS Size [bytes/block]"), ("scratch", "ScratchSize [bytes/lane]"),
        ("occ", "Occupancy [waves/SIMD]"))


def remarks(path):
    out, cur = {}, None
    for l in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", l)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def code(path):
    """mangled kernel name -> (size, sha1 of its bytes) from the gfx950 code object inside the host object"""
    data = open(path, "rb").read()
    out = {}
    for m in re.finditer(b"\x7fELF", data):
        blob = data[m.start():]
        if blob[18:20] != b"\xe0\x00":   # e_machine == EM_AMDGPU
            continue
        with tempfile.NamedTemporaryFile(suffix=".elf", delete=False) as f:
            f.write(blob)
        tmp = f.name
        sec = subprocess.run([f"{LLVM}/llvm-readelf", "-SW", tmp], capture_output=True, text=True).stdout
        t = re.search(r"\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", sec)
        addr, off = int(t.group(1), 16), int(t.group(2), 16)
        for l in subprocess.run([f"{LLVM}/llvm-readelf", "-sW", tmp], capture_output=True, text=True).stdout.splitlines():
            p = l.split()
            if len(p) >= 8 and p[3] == "FUNC":
                a, n = int(p[1], 16), int(p[2])
                out[p[7]] = (n, hashlib.sha1(blob[off + a - addr:off + a - addr + n]).hexdigest())
        os.unlink(tmp)
    return out


def demangle(n):
    return subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().split("(")[0].replace("crfp::", "").replace("crfp_bf16::", "")


def merged(read, paths):
    """one table from a comma-separated list of files: the kernels of a translation unit that was split stay comparable"""
    out = {}
    for p in paths.split(","):
        out.update(read(p))
    return out


args = sys.argv[1:]
for i in range(0, len(args), 5):
    label, o0, r0, o1, r1 = args[i:i + 5]
    R0, R1, C0, C1 = merged(remarks, r0), merged(remarks, r1), merged(code, o0), merged(code, o1)
    print(f"## {label}\n")
    print("| kernel | " + " | ".join(k for k, _ in KEYS) + " | code bytes | same ISA | same resources |\n|---|" + "---|" * (len(KEYS) + 3))
    for n in sorted(set(R0) | set(R1), key=demangle):
        a, b = R0.get(n), R1.get(n)
        if a is None or b is None:
            print(f"| {demangle(n)} | " + ("only in new" if a is None else "only in old") + " |" * (len(KEYS) + 3))
            continue
        cols = [a[k] if a[k] == b[k] else f"{a[k]} -> {b[k]}" for _, k in KEYS]
        s0, s1 = C0[n], C1[n]
        size = str(s0[0]) if s0[0] == s1[0] else f"{s0[0]} -> {s1[0]}"
        same = all(a[k] == b[k] for _, k in KEYS)
        print(f"| {demangle(n)} | " + " | ".join(cols) + f" | {size} | {'yes' if s0 == s1 else 'no'} | {'yes' if same else 'NO'} |")
    print()
