"""What the build of haghighatshoarmuir2024_amd/csrc says about itself, asked of make (csrc/Makefile derives its sources from the directory
and its header prerequisites from the compiler's .d files, so its text names neither), and the include closure read from the sources,
independent of make, to hold against it."""
import functools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
PUBLIC_HEADER = "../../include/micloc_hip.h"  # as the sources and the .d files spell it, seen from csrc/


def _make(*args):
    return subprocess.run(["make", "-C", CSRC, *args], capture_output=True, text=True, check=True).stdout


@functools.lru_cache(maxsize=None)
def built_sources():
    """The *.hip files whose objects the library is linked from."""
    line = re.search(r"^\.\./libmicloc_hip\.so:(.*)$", _make("-pn"), re.M).group(1)
    return frozenset(o[:-2] + ".hip" for o in line.split() if o.endswith(".o"))


@functools.lru_cache(maxsize=None)
def _up_to_date():
    _make("-s", "-j4")  # a no-op on a built tree; the .d files exist afterwards and every object is newer than its sources


def rebuilt_after_edit(header):
    """The objects make would compile again after an edit of `header` (a name in csrc/, or PUBLIC_HEADER)."""
    _up_to_date()
    return set(re.findall(r" -o (\S+\.o) ", _make("-n", "-W", header)))


def sources():
    """{file name: text} of csrc/*.hip and csrc/*.h, and of the public header under PUBLIC_HEADER."""
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
    src[PUBLIC_HEADER] = open(os.path.join(CSRC, PUBLIC_HEADER)).read()
    return src


def includes(src, f, seen=None):
    """Project headers f includes, directly or through another project header."""
    seen = set() if seen is None else seen
    for h in re.findall(r'#include "([^"]+)"', src[f]):
        if h in src and h not in seen:
            seen.add(h)
            includes(src, h, seen)
    return seen


def including_objects(header):
    """The objects whose sources include `header`, by the include closure."""
    src = sources()
    return {f[:-4] + ".o" for f in src if f.endswith(".hip") and header in includes(src, f)}
