#!/usr/bin/env python3
"""Are the objects of two builds of csrc/ the same code?   python tools/dev/cmp_objects.py <csrc of build A> <csrc of build B> [unit ...]

`cmp` cannot answer: clang names a few symbols of every HIP unit after a compilation-unit id, a hash of the source's absolute path and
of the whole command line, so the same source compiled in another directory, or with `-MMD` added, differs in those names and in the
symbol hash tables built from them.  Compared here, per object: the device code object's loaded sections (.note with the kernels'
metadata, .rodata with their descriptors, .text, .data) byte for byte, and of the host object every section but .hip_fatbin and the
string and symbol tables, and the symbols by name, with the id blanked.  Exit 1 if any unit differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
DEVICE_SECTIONS = (".note", ".rodata", ".text", ".data")


def run(*cmd):
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def parts(obj, tmp):
    """{name: bytes} of what an object says about the code it holds."""
    dump = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-s", "-t", obj], capture_output=True, text=True, check=True).stdout
    blocks = re.split(r"\n(?=Contents of section |SYMBOL TABLE:)", dump)[1:]  # (what stands before them names the file)
    host = "\n".join(b for b in blocks if not re.match(r"Contents of section (\.strtab|\.symtab|\.hip_fatbin):", b))
    m = re.search(r"__hip_cuid_([0-9a-f]+)", host)
    out = {"host": (host.replace(m.group(1), "<id>") if m else host).encode()}
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "device.co")
    run(os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    if os.path.getsize(fat) == 0:
        return out  # host code only
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}")
    have = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-S", "-W", co], capture_output=True, text=True).stdout
    for sec in DEVICE_SECTIONS:
        if re.search(r"\] " + re.escape(sec) + r"\s", have):
            dump = os.path.join(tmp, "section")
            run(os.path.join(LLVM, "llvm-objcopy"), f"--dump-section={sec}={dump}", co)
            out["device " + sec] = open(dump, "rb").read()
    return out


def main(a, b, units):
    units = units or sorted(f[:-2] for f in os.listdir(a) if f.endswith(".o"))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for u in units:
            pa, pb = (parts(os.path.join(d, u + ".o"), tmp) for d in (a, b))
            diff = sorted(k for k in pa.keys() | pb.keys() if pa.get(k) != pb.get(k))
            print(f"{u + '.o':28s}", "DIFFERS in " + ", ".join(diff) if diff else "same  (" + ", ".join(f"{k} {len(v)}" for k, v in pa.items()) + ")")
            bad += bool(diff)
    print(f"{len(units) - bad} of {len(units)} objects hold the same code")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
