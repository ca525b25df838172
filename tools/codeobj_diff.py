#!/usr/bin/env python3
"""Do two builds hold the same gfx950 kernels, byte for byte?

    tools/codeobj_diff.py --old OLD.o [OLD2.o ...] --new NEW1.o [NEW2.o ...] [--list]

Each argument is a host object compiled by hipcc (biahub_amd/build/<unit>.hip.o).  Its gfx950 code object is taken out of the
.hip_fatbin section (llvm-objcopy + clang-offload-bundler), and for every kernel (FUNC symbol with a `.kd` descriptor) the
machine code of its symbol range and its entry in the code-object metadata (VGPRs, SGPRs, LDS, scratch, kernarg size, ...) are
compared between the two sides.  Reported: kernels only on one side, kernels present in more than one object of a side, kernels
whose bytes or metadata differ.  Exit status 0 only when the two sides are identical.  Runs without a GPU."""
import hashlib
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import yaml

LLVM = Path("/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run([str(c) for c in cmd], check=True, capture_output=True, text=True).stdout


def code_object(obj: Path, tmp: Path) -> Path:
    fat, co = tmp / (obj.name + ".fatbin"), tmp / (obj.name + ".co")
    run(LLVM / "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    run(LLVM / "clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--targets={TARGET}", f"--output={co}")
    return co


def metadata(co: Path) -> dict:
    """kernel name -> its code-object metadata entry (registers, LDS, scratch, kernarg size, the argument list, ...)"""
    text = run(LLVM / "llvm-readelf", "--notes", co)
    doc = yaml.safe_load(text[text.index("amdhsa.kernels:"):text.index("\n...")])
    return {k[".name"]: {f: v for f, v in k.items() if f not in (".name", ".symbol")} for k in doc["amdhsa.kernels"]}


def kernels(co: Path) -> dict:
    """kernel name -> (sha256 of its code, size, metadata)"""
    data = co.read_bytes()
    sections = {}  # index -> (address, file offset)
    for line in run(LLVM / "llvm-readelf", "-SW", co).splitlines():
        m = re.match(r"^\s*\[\s*(\d+)\]\s+(\S*)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            sections[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))
    funcs, descriptors = {}, set()
    for line in run(LLVM / "llvm-readelf", "-sW", co).splitlines():
        f = line.split()
        if len(f) < 8 or not f[0].rstrip(":").isdigit():
            continue
        value, size, kind, ndx, name = int(f[1], 16), int(f[2]), f[3], f[6], f[7]
        if kind == "FUNC" and ndx.isdigit():
            addr, off = sections[int(ndx)]
            funcs[name] = data[off + value - addr: off + value - addr + size]
        elif kind == "OBJECT" and name.endswith(".kd"):
            descriptors.add(name[:-3])
    meta = metadata(co)
    return {n: (hashlib.sha256(b).hexdigest(), len(b), meta.get(n, {})) for n, b in funcs.items() if n in descriptors}


def side(objs, tmp, label, problems):
    merged, where = {}, {}
    for o in objs:
        for name, k in kernels(code_object(Path(o), tmp)).items():
            if name in merged:
                problems.append(f"{label}: kernel in two objects ({where[name]}, {Path(o).name}): {name}")
            merged[name], where[name] = k, Path(o).name
    return merged, where


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=str(LLVM))
    if not names or not filt:
        return {n: n for n in names}
    res = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, res.stdout.splitlines()))


def main(argv):
    if "--old" not in argv or "--new" not in argv:
        sys.exit(__doc__)
    show = "--list" in argv
    argv = [a for a in argv if a != "--list"]
    i, j = argv.index("--old"), argv.index("--new")
    old_objs, new_objs = (argv[i + 1:j], argv[j + 1:]) if i < j else (argv[i + 1:], argv[j + 1:i])
    problems = []
    with tempfile.TemporaryDirectory() as t:
        old, _ = side(old_objs, Path(t), "old", problems)
        new, where = side(new_objs, Path(t), "new", problems)
    for n in sorted(set(old) - set(new)):
        problems.append(f"lost: {n}")
    for n in sorted(set(new) - set(old)):
        problems.append(f"added ({where[n]}): {n}")
    same = 0
    for n in sorted(set(old) & set(new)):
        (ho, so, mo), (hn, sn, mn) = old[n], new[n]
        if ho != hn:
            problems.append(f"code differs ({so} -> {sn} bytes, {where[n]}): {n}")
        elif mo != mn:
            keys = sorted(k for k in set(mo) | set(mn) if mo.get(k) != mn.get(k))
            problems.append(f"metadata differs ({', '.join(f'{k}: {mo.get(k)} -> {mn.get(k)}' for k in keys)}): {n}")
        else:
            same += 1
    per_obj = {}
    for n, (_, size, _) in new.items():
        c = per_obj.setdefault(where[n], [0, 0])
        c[0] += 1
        c[1] += size
    print(f"old: {len(old)} kernels in {len(old_objs)} object(s), {sum(k[1] for k in old.values())} bytes of kernel code")
    print(f"new: {len(new)} kernels in {len(new_objs)} object(s), {sum(k[1] for k in new.values())} bytes of kernel code")
    for o in sorted(per_obj):
        print(f"  {o}: {per_obj[o][0]} kernels, {per_obj[o][1]} bytes")
    print(f"identical code and metadata: {same}")
    names = demangle([p.rsplit(": ", 1)[1] for p in problems])
    for p in problems:
        head, n = p.rsplit(": ", 1)
        print(f"{head}: {names.get(n, n)}")
    if show:
        dm = demangle(sorted(new))
        for n in sorted(new):
            m = new[n][2]
            print(f"{new[n][0][:16]} {new[n][1]:7d} B  vgpr {m.get('.vgpr_count')} sgpr {m.get('.sgpr_count')} lds {m.get('.group_segment_fixed_size')} "
                  f"scratch {m.get('.private_segment_fixed_size')} kernarg {m.get('.kernarg_segment_size')}  {dm[n]}")
    print("RESULT:", "IDENTICAL" if not problems else f"{len(problems)} finding(s)")
    return 0 if not problems else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
