#!/usr/bin/env python3
"""The compiler and flags csrc/Makefile uses for one unit of the library, asked of make itself (nothing here restates a flag).

    python tools/make_cmd.py xylo        prints: /opt/rocm/bin/hipcc -O3 ... -mllvm -amdgpu-mfma-vgpr-form

A dry run that forces the object prints the exact command, target-specific flags included; what follows the flags in it
(-MMD -MP -c -o <unit>.o <unit>.hip) is the caller's to say: a variant names its own source and object, an ISA dump adds
--cuda-device-only -S.  Environment and `EXTRA=` reach make as in a build."""
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")


def compiler_and_flags(unit):
    """[compiler, flag, ...] of `unit`.o as the Makefile compiles it."""
    line = subprocess.run(["make", "-s", "-n", "-B", "-C", CSRC, unit + ".o"], capture_output=True, text=True, check=True).stdout.strip()
    args = shlex.split(line)
    tail = ["-MMD", "-MP", "-c", "-o", unit + ".o", unit + ".hip"]
    if "\n" in line or args[-len(tail):] != tail:
        raise SystemExit(f"make_cmd: csrc/Makefile compiles {unit}.o by something other than one command ending in `{' '.join(tail)}`:\n{line}")
    return args[:-len(tail)]


if __name__ == "__main__":
    print(" ".join(shlex.quote(a) for a in compiler_and_flags(sys.argv[1])))
