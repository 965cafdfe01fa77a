#!/usr/bin/env python3
"""Compares the instruction text of kernels in two builds of libmicloc_hip.so: every gfx950 code object of the library's .hip_fatbin
section is unbundled and disassembled (llvm-objdump -d, demangled, without addresses and encodings), and the kernels whose demangled
name matches PATTERN are compared instruction by instruction -- the check that a change which moves shared code leaves an existing kernel
as it was.  Exit status 0 when every matching kernel of OLD exists in NEW with the same text.

    python tools/dev/kernel_text_diff.py OLD/libmicloc_hip.so NEW/libmicloc_hip.so [--pattern REGEX] [--show NAME]

--show NAME prints the unified diff of the first kernel whose name contains NAME.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
DEFAULT = r"xylo_lif_pk_kernel<|xylo_lif_kernel<|xylo_lif_stream_kernel<|xylo_lif_track\w*_kernel<"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels(lib):
    """demangled symbol -> list of instructions, over every code object of the library"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        sec = os.path.join(d, "fatbin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, sec])
        data = open(sec, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]  # one bundle per translation unit
        for i, s in enumerate(starts):
            bundle, co = os.path.join(d, f"b{i}"), os.path.join(d, f"co{i}")
            with open(bundle, "wb") as f:
                f.write(data[s : starts[i + 1] if i + 1 < len(starts) else len(data)])
            subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={bundle}", f"--output={co}",
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], stderr=subprocess.DEVNULL)
            asm = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
            name = None
            for line in asm.splitlines():
                line = line.strip()
                m = re.match(r"^[0-9a-f]* ?<(.*)>:$", line)
                if m:
                    name = m.group(1)
                    out[name] = []
                elif name is not None and line:
                    out[name].append(re.sub(r"\s*//.*$", "", line))  # (the comment holds the absolute address of a branch target)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--pattern", default=DEFAULT)
    ap.add_argument("--show", default=None)
    args = ap.parse_args(argv)
    pat = re.compile(args.pattern)
    a, b = kernels(args.old), kernels(args.new)
    names = sorted(n for n in a if pat.search(n))
    same = bool(names)
    for n in names:
        short = n.split("(")[0]
        if n not in b:
            print(f"MISSING in new: {short}")
            same = False
            continue
        eq = a[n] == b[n]
        same &= eq
        print(f"{'identical' if eq else 'DIFFERENT'} {len(a[n]):6d} -> {len(b[n]):6d} instructions  {short}")
    for n in sorted(n for n in b if pat.search(n) and n not in a):
        print(f"new: {len(b[n]):6d} instructions  {n.split('(')[0]}")
    if args.show:
        hit = [n for n in names if args.show in n and n in b]
        if hit:
            print("\n".join(difflib.unified_diff(a[hit[0]], b[hit[0]], lineterm="", n=2)))
    print(f"{len(names)} kernels compared: " + ("ALL IDENTICAL" if same else "NOT IDENTICAL"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
